// tests/test_g711_cpu.py: the library's G.711 arithmetic (rnnoise_amd/csrc/g711.h, the text K0 and K3 compile) over every input, on
// the host.  Writes to stdout, raw: 65,536 mu-law codes of x = -32768 .. 32767, 65,536 A-law codes, 256 mu-law values as little-endian
// int16, 256 A-law values.
#include <stdint.h>
#include <stdio.h>

#include "../../rnnoise_amd/csrc/g711.h"

int main() {
  static uint8_t enc[2][65536];
  static int16_t dec[2][256];
  for (int x = -32768; x < 32768; x++) {
    enc[0][x + 32768] = (uint8_t)rn_g711_encode(RN_PCM_ULAW, x);
    enc[1][x + 32768] = (uint8_t)rn_g711_encode(RN_PCM_ALAW, x);
  }
  for (int b = 0; b < 256; b++) {
    dec[0][b] = (int16_t)rn_g711_decode(RN_PCM_ULAW, b);
    dec[1][b] = (int16_t)rn_g711_decode(RN_PCM_ALAW, b);
  }
  return fwrite(enc, 1, sizeof enc, stdout) == sizeof enc && fwrite(dec, 1, sizeof dec, stdout) == sizeof dec ? 0 : 1;
}
