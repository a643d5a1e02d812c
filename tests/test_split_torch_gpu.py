"""The split calls from torch (rnnoise_amd/torch_op.py: torch.ops.rnnoise_amd.analyze / synthesize, RNNoiseOp.denoise_with) and from
the command line (cli denoise --torch-net), on a small scripted GRU that maps [N, T, 65] to ([N, T, 32], [N, T, 1]):

  a  the registered ops on CUDA tensors, on torch's current stream, with the batch's own network between them (process_features_device
     on the batch-first rows): the bits of torch.ops.rnnoise_amd.process; the fake kernels' shapes
  b  denoise_with(net, pcm) against the split oracle (tests/csrc/split_oracle.c) fed the same module's outputs
  c  cli denoise --torch-net FILE.pt against denoise_with, and the --max-store-gb refusal
"""
import numpy as np
import pytest

from conftest import assert_bits_equal, load_blob
from rnnoise_amd import capi, cli, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
IDS = [3, 77, 130, 9, 20]


class TinyNet(torch.nn.Module):
    """a stateless-across-calls GRU: features [N, T, 65] -> (gains [N, T, 32], vad [N, T, 1]), both in (0, 1)"""

    def __init__(self):
        super().__init__()
        self.gru = torch.nn.GRU(65, 24, batch_first=True)
        self.gains = torch.nn.Linear(24, 32)
        self.vad = torch.nn.Linear(24, 1)

    def forward(self, x):
        h, _ = self.gru(x)
        return torch.sigmoid(self.gains(h)), torch.sigmoid(self.vad(h))


@pytest.fixture(scope="module")
def net():
    torch.manual_seed(7)
    return torch.jit.script(TinyNet().eval()).cuda()


def test_registered_ops_with_the_batchs_own_network():
    from rnnoise_amd.torch_op import RNNoiseOp
    blob, T, n = load_blob("default"), 7, len(IDS)
    pcm = synth.batch_pcm(IDS, T)
    x = torch.from_numpy(pcm).cuda()
    whole, op = RNNoiseOp(blob, n), RNNoiseOp(blob, n)
    w_out, w_vad, w_gains = whole(x)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        feats, sil = torch.ops.rnnoise_amd.analyze(x, op.state, op.handle)
        assert feats.shape == (n, T, 65) and sil.shape == (T, n) and sil.dtype == torch.int32
        gains, vad = torch.empty((n, T, 32), device="cuda"), torch.empty((n, T, 1), device="cuda")
        # (process_features writes [T][N] rows: staged there, then handed over batch-first)
        g_tn, v_tn = torch.empty((T, n, 32), device="cuda"), torch.empty((T, n), device="cuda")
        op.batch.process_features_device(g_tn.data_ptr(), v_tn.data_ptr(), feats.data_ptr(), T, frame_stride=65, row_stride=T * 65,
                                         stream=st.cuda_stream)
        gains.copy_(g_tn.transpose(0, 1)), vad.copy_(v_tn.t().unsqueeze(-1))
        out = torch.ops.rnnoise_amd.synthesize(gains, vad, x, op.state, op.handle)
    st.synchronize()
    assert not sil.cpu().numpy().any() and op.batch.split_pending == 0 and int(op.state.item()) == T
    assert_bits_equal(out.cpu().numpy(), w_out.cpu().numpy(), "out against torch.ops.rnnoise_amd.process")
    assert_bits_equal(g_tn.cpu().numpy(), w_gains.cpu().numpy(), "gains")
    with torch._subclasses.fake_tensor.FakeTensorMode():
        state = torch.zeros(1, dtype=torch.int64, device="cuda")
        ff, fs = torch.ops.rnnoise_amd.analyze(torch.empty((3, n, 480), device="cuda"), state, op.handle)
        assert ff.shape == (n, 3, 65) and fs.shape == (3, n) and fs.dtype == torch.int32
        fo = torch.ops.rnnoise_amd.synthesize(torch.empty((n, 3, 32), device="cuda"), torch.empty((n, 3, 1), device="cuda"),
                                              torch.empty(0, dtype=torch.int16, device="cuda"), state, op.handle)
        assert fo.shape == (3, n, 480) and fo.dtype == torch.int16
    op.close(), whole.close()


def test_denoise_with_a_scripted_gru_against_the_split_oracle(net):
    from rnnoise_amd.torch_op import RNNoiseOp
    from split_oracle import SplitStream
    blob, T, n = load_blob("default"), 9, len(IDS)
    pcm = synth.batch_pcm(IDS, T, lead_silence=2)
    op = RNNoiseOp(blob, n)
    x = torch.from_numpy(pcm).cuda()
    out = op.denoise_with(net, x).cpu().numpy()
    # the module's outputs on the exported features, which are the oracle's own on every frame that is not silent
    op.reset()
    feats, sil = op.analyze(x)
    with torch.no_grad():
        gains, vad = net(feats)
    again = op.synthesize(gains, vad).cpu().numpy()
    assert_bits_equal(again, out, "denoise_with against the three steps by hand")
    gains, vad, sil = gains.cpu().numpy(), vad.cpu().numpy(), sil.cpu().numpy()
    assert sil[:2].all() and not sil[2:].any()
    for s in range(n):
        o = SplitStream()
        ofeats, osil = o.analyze(pcm[:, s])
        assert_bits_equal(feats[s, 2:].cpu().numpy(), ofeats[2:], f"stream {s}: exported features")
        assert_bits_equal(out[:, s], o.synthesize(gains[s], vad[s, :, 0]), f"stream {s}: out against the split oracle")
    op.close()


def test_cli_torch_net_against_denoise_with(net, tmp_path):
    from rnnoise_amd.torch_op import RNNoiseOp
    blob = load_blob("default")
    lens = [30 * 480 + 77, 12 * 480]
    paths = []
    for s, m in enumerate(lens):
        x = synth.stream_pcm(20 + s, m // 480 + 1)[:m]
        p = tmp_path / f"in{s}.raw"
        x.tofile(p)
        paths.append(str(p))
    (tmp_path / "w.blob").write_bytes(blob)
    net.save(str(tmp_path / "net.pt"))
    args = ["denoise", "--model", str(tmp_path / "w.blob"), "--out-dir", str(tmp_path / "out"), "--torch-net", str(tmp_path / "net.pt")]
    cli.main(args + paths)
    # the same group through the function: the shorter file is fed silence to the longer one's length
    T = max(lens) // 480
    pcm = np.zeros((T, len(lens), 480), np.int16)
    for s, m in enumerate(lens):
        k = m // 480
        pcm[:k, s] = np.fromfile(paths[s], dtype=np.int16)[:k * 480].reshape(k, 480)
    op = RNNoiseOp(blob, len(lens), nn_path="vector")
    want = op.denoise_with(net, torch.from_numpy(pcm).cuda()).cpu().numpy()
    assert want.dtype == np.int16
    for s, m in enumerate(lens):
        k = m // 480
        got = np.fromfile(tmp_path / "out" / f"in{s}.raw.denoised.raw", dtype=np.int16)
        assert got.size == (k - 1) * 480
        assert np.array_equal(got, want[1:k, s].reshape(-1)), f"file {s}"
    op.close()
    # a store above the limit is refused before anything runs
    with pytest.raises(ValueError, match="max-store-gb"):
        cli.main(args + ["--max-store-gb", str(0.5 * capi.split_frame_bytes(2) * T / 2 ** 30)] + paths)
