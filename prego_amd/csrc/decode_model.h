// The quantiser and the model words of the Viterbi kernels (decode.hip: whole videos; decode_pool.hip: live streams, a frame at a time):
// one copy of the table and of the three clamps, so that both decode the same costs to the bit.
#pragma once
#include "kernels.h"

// LUT[k] = rint(256 * log2(1 + (k + 0.5) / 256)): the only copy on the device (prego_amd/decode.py holds the host's)
static __device__ const unsigned short kDecodeLut[256] = {
      1,   2,   4,   5,   6,   8,   9,  11,  12,  13,  15,  16,  18,  19,  20,  22,
     23,  24,  26,  27,  28,  30,  31,  32,  34,  35,  36,  38,  39,  40,  42,  43,
     44,  45,  47,  48,  49,  50,  52,  53,  54,  55,  57,  58,  59,  60,  62,  63,
     64,  65,  66,  68,  69,  70,  71,  72,  74,  75,  76,  77,  78,  80,  81,  82,
     83,  84,  85,  86,  88,  89,  90,  91,  92,  93,  94,  95,  97,  98,  99, 100,
    101, 102, 103, 104, 105, 106, 108, 109, 110, 111, 112, 113, 114, 115, 116, 117,
    118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 131, 132, 133, 134,
    135, 136, 137, 138, 139, 140, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149,
    150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 162, 163, 163, 164,
    165, 166, 167, 168, 169, 170, 171, 172, 173, 173, 174, 175, 176, 177, 178, 179,
    180, 181, 182, 182, 183, 184, 185, 186, 187, 188, 189, 189, 190, 191, 192, 193,
    194, 195, 195, 196, 197, 198, 199, 200, 200, 201, 202, 203, 204, 205, 205, 206,
    207, 208, 209, 210, 210, 211, 212, 213, 214, 214, 215, 216, 217, 218, 218, 219,
    220, 221, 222, 222, 223, 224, 225, 226, 226, 227, 228, 229, 229, 230, 231, 232,
    233, 233, 234, 235, 236, 236, 237, 238, 239, 239, 240, 241, 242, 242, 243, 244,
    245, 245, 246, 247, 248, 248, 249, 250, 251, 251, 252, 253, 253, 254, 255, 256};

// the emission cost of the fp32 word w (include/prego_amd.h, "Emission cost of a probability"); lut: kDecodeLut or its copy in LDS
__device__ __forceinline__ int dec_cost_of_prob(unsigned w, const unsigned short* lut) {
  const unsigned e = (w >> 23) & 0xFFu, k = (w >> 15) & 0xFFu;
  const int c = 256 * (127 - (int)e) - (int)lut[k];
  const bool bad = (w >> 31) != 0u || e == 0u || (e == 255u && (w & 0x7FFFFFu) != 0u);
  return bad ? kDecodeCap : (e >= 127u ? 0 : c);
}
// a cost word of the caller's (costs mode): clamped into [0, CAP]
__device__ __forceinline__ int dec_cost_of_word(unsigned w) {
  const int c = (int)w;
  return c < 0 ? 0 : (c > kDecodeCap ? kDecodeCap : c);
}
// a word of trans / init: negative = forbidden (-1), above CAP = CAP
__device__ __forceinline__ int dec_model_word(int w) { return w < 0 ? -1 : (w > kDecodeCap ? kDecodeCap : w); }
