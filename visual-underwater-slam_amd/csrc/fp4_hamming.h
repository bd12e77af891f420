// fp4_hamming.h -- what the two all-pairs Hamming kernels on the matrix cores share: the track matcher
// (hamming_match_mfma_kernel, match.hip) and the keyframe retrieval (keyframe_similarity_kernel, retrieve.hip).
//
// With the descriptor bits as +-1 values, dot(q, t) = 256 - 2 * Hamming(q, t) exactly.  +-1 is exact in FP4 (E2M1:
// +1.0 = 0x2, -1.0 = 0xA), so the product runs on the block-scaled FP4 MFMA v_mfma_scale_f32_32x32x64_f8f6f4: four MFMAs
// per 32x32 tile over K = 256.  A and B use the same lane -> k map (MFMA ks, lane half h <-> descriptor word 2 ks + h), so
// only the C layout (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) matters.
//
// Internal linkage, like frontend_common.h: every unit that includes it gets its own copy.
#pragma once
#include <cstdint>

namespace {

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef float v16f_t __attribute__((ext_vector_type(16)));

constexpr int HM_ROWB = 144;             // bytes per expanded row: 128 + 16 (bank spread of the b128 reads)
constexpr int HM_SCALE_A = 0x7F7F7F7F;   // E8M0 block scales, every byte the same: 2^0

// 8 descriptor bits (the low byte of b) -> 8 FP4 nibbles, -1.0 (0xA) for a set bit and +1.0 (0x2) for a clear one.
// The sign is flipped for both operands alike, so every product is unchanged.
__device__ __forceinline__ int spread_fp4(uint32_t b) {
  uint32_t x = (b | b << 12) & 0x000F000Fu;         // bits 0-3 -> 0-3, bits 4-7 -> 16-19
  x = (x | x << 6) & 0x03030303u;                   // bit pairs -> bits 0-1 of each byte
  return (int)(((x << 3 | x << 6) & 0x88888888u) | 0x22222222u);   // bit 0 -> 3, bit 1 -> 7: sign bits of the nibbles
}

// one descriptor word (32 bits) -> the 32 FP4 values of one lane's operand of one MFMA: four lookups in the block's
// 256-entry byte table (one v_lshlrev_b32_sdwa + one ds_read_b32 per byte instead of eight VALU instructions)
__device__ __forceinline__ v4i_t spread_word(const uint32_t* lut, uint32_t w) {
  return v4i_t{(int)lut[w & 0xFFu], (int)lut[(w >> 8) & 0xFFu], (int)lut[(w >> 16) & 0xFFu], (int)lut[w >> 24]};
}

__device__ __forceinline__ v8i_t fp4_operand(v4i_t v) {   // FP4 reads dwords 0-3 of the builtin's 8-dword operand
  return v8i_t{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
}

}  // namespace
