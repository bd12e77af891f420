// orient.hip -- intensity-centroid orientation + rotated BRIEF of the stereo ORB front-end (frontend_common.h).
//
// Design notes (MI355X):
//  * orient_rbrief uses one 64-lane wave per keypoint: lane-strided disc moments, integer bin
//    choice, and the descriptor words come straight out of __ballot (lane = test bit).
#include "frontend_common.h"
#include <type_traits>
#define VUS_TABLE_QUAL __device__ constexpr
#include "../../include/vus_orb_tables.h"
#include "../../include/vus_tiled.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Orientation bin + 256-bit rotated BRIEF: one wave serves eight keypoints of one image (orient_rbrief_kernel below).
// Their 31-row centroid patches of the image are weighed in the registers they are loaded into; their 37-row patches of
// the smoothed image pass through LDS one at a time for the 256 byte-pair tests.  The planes are row-major or
// block-tiled (OrGeom).  The section's two build knobs, occupancy over identical code:
#ifndef VUS_OR_WPE
#define VUS_OR_WPE 4         // waves per SIMD asked of the compiler for the row-major instances
#endif
#ifndef VUS_OR_WPE_TILED
#define VUS_OR_WPE_TILED 7   // ... for the tiled instances; tests/test_orient_resources.py holds what 7 takes
#endif
constexpr int OR_R = 15;                    // disc radius
constexpr int OR_ROWS = 2 * OR_R + 1;       // 31
constexpr int OR_DW = 10;                   // 36 bytes cover x-15..x+15 from an aligned start; whole dwordx2 are loaded
constexpr int BR_R = VUS_RBRIEF_REACH;      // 18
constexpr int BR_ROWS = 2 * BR_R + 1;       // 37
constexpr int BR_DW = 10;                   // 40 bytes cover x-18..x+18 from an aligned start
constexpr int BR_DW_TILED = 12;             // block-tiled planes: 44 of 48 bytes from an 8-byte aligned start (OrGeom)
constexpr int OR_KP_PER_WAVE = 8;           // keypoints of one wave; the reduce-scatter and the one-store epilogue are written for 8

// Load a (2*RADIUS+1) x (4*DW)-byte patch around (x, y) into registers: every lane issues all of
// its loads back to back (one memory round trip), the caller stores them to LDS afterwards.
// A lane moves two dwords per load (dwordx2 at dword alignment): the texture path's cost is per instruction, not per
// byte.  Measured and not kept, ms per 1000 frames against the 2.82 of 6 dwordx2 per keypoint: 11 dword loads: 3.19;
// 4 dwordx4 of 48-byte rows: 3.04.
typedef uint32_t PatchVec __attribute__((ext_vector_type(2), aligned(1)));

// EXACT: the patch starts at column x - RADIUS whatever its alignment (images whose rows are not dword
// aligned, e.g. odd-width pyramid levels); otherwise at the dword boundary below it (aligned loads are
// ~7 % faster on the full-size image: 2.70 vs 2.90 ms per 1000 frames).
template <int RADIUS, int DW, bool EXACT>
struct PatchRegs {
  static_assert(DW % 2 == 0, "row width must be a multiple of the vector width");
  static constexpr int ROWS = 2 * RADIUS + 1;
  static constexpr int HW = DW / 2;             // vectors per row
  static constexpr int N = ROWS * HW;
  static constexpr int ITERS = (N + 63) / 64;
  PatchVec v[ITERS];
  uint32_t off[ITERS];   // byte offset of this lane's vectors inside an in-image patch (fixed per kernel); unsigned:
                         // scalar base + zero-extended 32-bit lane offset is an addressing mode of global_load

  __device__ __forceinline__ void init(int pitch, int lane) {
#pragma unroll
    for (int u = 0; u < ITERS; ++u) {
      const int t = min(lane + 64 * u, N - 1);
      off[u] = (uint32_t)((t / HW) * pitch + 8 * (t % HW));
    }
  }
  __device__ __forceinline__ void load(const uint8_t* __restrict__ src, int H, int W, int pitch, int y, int x,
                                       int lane) {
    const int xa = EXACT ? x - RADIUS : (x - RADIUS) & ~3;   // start column
    const bool inside = y - RADIUS >= 0 && y + RADIUS < H && xa >= 0 && xa + 4 * DW <= W;
    if (inside) {   // wave-uniform
      const uint8_t* base = src + (size_t)(y - RADIUS) * pitch + xa;
#pragma unroll
      for (int u = 0; u < ITERS; ++u) v[u] = *reinterpret_cast<const PatchVec*>(base + (size_t)off[u]);
    } else {        // replicate-clamped, byte by byte (keypoints near the image edge)
#pragma unroll
      for (int u = 0; u < ITERS; ++u) {
        const int t = min(lane + 64 * u, N - 1);
        const int r = t / HW, c = t - r * HW;
        const uint8_t* rp = src + (size_t)clampi(y - RADIUS + r, 0, H - 1) * pitch;
        const int gx = xa + 8 * c;
#pragma unroll
        for (int k = 0; k < 2; ++k)
          v[u][k] = (uint32_t)rp[clampi(gx + 4 * k, 0, W - 1)] | ((uint32_t)rp[clampi(gx + 4 * k + 1, 0, W - 1)] << 8) |
                    ((uint32_t)rp[clampi(gx + 4 * k + 2, 0, W - 1)] << 16) |
                    ((uint32_t)rp[clampi(gx + 4 * k + 3, 0, W - 1)] << 24);
      }
    }
  }
  __device__ __forceinline__ void store(uint32_t* __restrict__ dst, int lane) const {
#pragma unroll
    for (int u = 0; u < ITERS; ++u)
      if (lane + 64 * u < N) *reinterpret_cast<uint2*>(dst + 2 * (lane + 64 * u)) = make_uint2(v[u][0], v[u][1]);
  }
};

// The same patch, and the same interface, from a block-tiled plane (include/vus_tiled.h; W % 16 == 0, H % 8 == 0, the
// pitch is W and goes unused).  The patch starts at the 8-byte boundary below x - RADIUS, so a lane's dwordx2 never
// leaves a 16-byte block row.  Pixel (y0 + r, xa + 8 c) of vector (r, c) sits at
//   tiled(y0 & ~7, xa & ~15)  +  16 (y0 & 7) + 16 r + f(q)  +  (p >> 3) (8 W - 128),   p = (y0 & 7) + r,  q = (xa & 8) + 8 c,
//   f(q) = 128 (q >> 4) + (q & 8)
// -- the first two terms wave-uniform, 16 r + f(q) a per-lane constant for each of the two values of xa & 8: four
// vector instructions per vector (add, shift, bit-field extract, multiply-add) on top of the plain form's load.  The
// three per-lane constants of a vector share ONE register (pk below): 6 bits of row, two 10-bit offsets.
template <int RADIUS, int DW>
struct TiledPatchRegs {
  static_assert(DW % 2 == 0, "row width must be a multiple of the vector width");
  static constexpr int ROWS = 2 * RADIUS + 1;
  static constexpr int HW = DW / 2;             // vectors per row
  static constexpr int N = ROWS * HW;
  static constexpr int ITERS = (N + 63) / 64;
  static_assert(ROWS + 7 < 64 && 16 * (ROWS - 1) + 128 * ((8 * HW) >> 4) + 8 < 1024, "pk fields: 6-bit row, 10-bit offsets");
  PatchVec v[ITERS];
  uint32_t pk[ITERS];   // this lane's vectors: (patch row r) << 20 | (16 r + f(q), xa & 8 == 8) << 10 | (..., xa & 8 == 0)

  __device__ __forceinline__ void init(int /*pitch*/, int lane) {
#pragma unroll
    for (int u = 0; u < ITERS; ++u) {
      const int t = min(lane + 64 * u, N - 1);
      const uint32_t r = (uint32_t)(t / HW), q0 = 8u * (uint32_t)(t % HW), q8 = q0 + 8u;
      const uint32_t off0 = 16u * r + 128u * (q0 >> 4) + (q0 & 8u), off8 = 16u * r + 128u * (q8 >> 4) + (q8 & 8u);
      pk[u] = r << 20 | off8 << 10 | off0;
    }
  }
  __device__ __forceinline__ void load(const uint8_t* __restrict__ src, int H, int W, int /*pitch*/, int y, int x,
                                       int lane) {
    const int xa = (x - RADIUS) & ~7, y0 = y - RADIUS;
    const bool inside = y0 >= 0 && y + RADIUS < H && xa >= 0 && xa + 4 * DW <= W;
    if (inside) {   // wave-uniform
      const uint8_t* base = src + vus_tiled_offset(y0 & ~7, xa & ~15, W) + 16 * (y0 & 7);
      const uint32_t ys = (uint32_t)(y0 & 7) << 20, ystep = 8u * (uint32_t)W - 128u;
      const uint32_t sel = (xa & 8) != 0 ? 10u : 0u;
#pragma unroll
      for (int u = 0; u < ITERS; ++u) {   // (ys + r) >> 3 == (pk + ys) >> 23: the row field has room for ys + r < 64
        const uint32_t off = ((pk[u] + ys) >> 23) * ystep + __builtin_amdgcn_ubfe(pk[u], sel, 10u);
        v[u] = *reinterpret_cast<const PatchVec*>(base + (size_t)off);
      }
    } else {        // replicate-clamped, byte by byte (keypoints near the image edge)
#pragma unroll
      for (int u = 0; u < ITERS; ++u) {
        const int t = min(lane + 64 * u, N - 1);
        const int r = t / HW, c = t - r * HW;
        const int gy = clampi(y0 + r, 0, H - 1), gx = xa + 8 * c;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          uint32_t w = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) w |= (uint32_t)src[vus_tiled_offset(gy, clampi(gx + 4 * k + b, 0, W - 1), W)] << (8 * b);
          v[u][k] = w;
        }
      }
    }
  }
  __device__ __forceinline__ void store(uint32_t* __restrict__ dst, int lane) const {
#pragma unroll
    for (int u = 0; u < ITERS; ++u)
      if (lane + 64 * u < N) *reinterpret_cast<uint2*>(dst + 2 * (lane + 64 * u)) = make_uint2(v[u][0], v[u][1]);
  }
};

// Cross-lane helpers of orient_rbrief_kernel.  A wave works on EIGHT keypoints at once; the per-lane
// partial sums of their centroid moments (16 values) are folded with a reduce-scatter instead of 16 full wave
// reductions: v_permlane32_swap / v_permlane16_swap (gfx950) exchange half-waves / odd-even rows of TWO registers in one
// instruction, so that one add folds two values at once; then one row_ror:8 and three 8-lane all-reduce steps.
// After it the eight lanes 8g..8g+7 hold the totals of keypoint g.
__device__ __forceinline__ int fold32(int x, int y) {   // lanes < 32: x[l] + x[l+32];  lanes >= 32: y[l-32] + y[l]
  auto r = __builtin_amdgcn_permlane32_swap((uint32_t)x, (uint32_t)y, false, false);
  return (int)(r[0] + r[1]);
}
__device__ __forceinline__ int fold16(int x, int y) {   // rows 0, 2: x's row pair summed;  rows 1, 3: y's row pair summed
  auto r = __builtin_amdgcn_permlane16_swap((uint32_t)x, (uint32_t)y, false, false);
  return (int)(r[0] + r[1]);
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
constexpr int DPP_ROW_ROR8 = 0x128, DPP_HALF_MIRROR = 0x141, DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E;
__device__ __forceinline__ int fold8(int x, int y, bool upper8) {   // lanes with bit 3 clear: x over lane pairs (l, l+8); set: y
  const int keep = upper8 ? y : x, give = upper8 ? x : y;
  return keep + dpp_i32<DPP_ROW_ROR8>(give);
}
__device__ __forceinline__ int allsum8(int v) {   // every lane: the sum over its group of eight lanes
  v += dpp_i32<DPP_HALF_MIRROR>(v);
  v += dpp_i32<DPP_QUAD_XOR1>(v);
  v += dpp_i32<DPP_QUAD_XOR2>(v);
  return v;
}
template <int CTRL>
__device__ __forceinline__ long long dpp_max_i64(long long key) {   // every source lane of these patterns exists
  const int lo = dpp_i32<CTRL>((int)(uint32_t)key), hi = dpp_i32<CTRL>((int)(key >> 32));
  const long long ok = (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
  return ok > key ? ok : key;
}
__device__ __forceinline__ long long allmax8_i64(long long key) {
  key = dpp_max_i64<DPP_HALF_MIRROR>(key);
  key = dpp_max_i64<DPP_QUAD_XOR1>(key);
  key = dpp_max_i64<DPP_QUAD_XOR2>(key);
  return key;
}

// v_writelane_b32: one lane of a register takes a wave-uniform value (no builtin in this compiler).  Value and lane
// select are both scalar registers and gfx9 encodings read ONE over the constant bus: the select goes through M0, which
// the instruction accepts as its lane operand.  M0 is written and consumed inside the one asm statement; no kernel of
// this file gives the compiler a reason to keep a value of its own there (no LDS-DMA, no indirect register indexing).
__device__ __forceinline__ uint32_t writelane_u32(uint32_t reg, uint32_t value, int lane_sel) {
  asm("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(reg) : "s"(value), "s"(lane_sel));   // M0 is a reserved register: not listable as a clobber
  return reg;
}

// A lane ranks the four bins 4 (lane & 7) + q after phase A: their directions, from the two per-bin tables.
__device__ __forceinline__ void load_bin_directions(const int (&cos_table)[VUS_N_ANGLE_BINS], const int (&sin_table)[VUS_N_ANGLE_BINS],
                                                    int lane, int (&bin_cos)[4], int (&bin_sin)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int bq = min(4 * (lane & 7) + q, VUS_N_ANGLE_BINS - 1);
    bin_cos[q] = cos_table[bq];
    bin_sin[q] = sin_table[bq];
  }
}

// Rotated test pattern re-laid for the kernel: [bin][lane][word] = the two patch byte offsets
// (y * row bytes + x, int16 each) of test 64 * word + lane.  Derived from VUS_RBRIEF_ROT at COMPILE time, so
// the table is part of the code object: no initialisation launch, nothing to order between streams or threads.
struct RotOffTable {
  uint32_t v[VUS_N_ANGLE_BINS * 64 * 4];
};
constexpr RotOffTable make_rot_off_table(int row_bytes) {
  RotOffTable r{};
  for (int e = 0; e < VUS_N_ANGLE_BINS * 256; ++e) {
    const int bin = e / 256, test = e - 256 * bin, w = test >> 6, lane = test & 63;
    const int oa = VUS_RBRIEF_ROT[4 * e + 1] * row_bytes + VUS_RBRIEF_ROT[4 * e];
    const int ob = VUS_RBRIEF_ROT[4 * e + 3] * row_bytes + VUS_RBRIEF_ROT[4 * e + 2];
    r.v[(bin * 64 + lane) * 4 + w] = ((uint32_t)oa & 0xFFFFu) | ((uint32_t)ob << 16);
  }
  return r;
}
// The tables of this unit start on a 128-byte line: a wave reads them 16 bytes per lane, 1024 contiguous bytes = eight
// lines, nine from any other start (orient_rbrief 1.714 against 1.697 ms per 1000 stereo frames with the 64-byte start
// the linker happened to give).
__device__ __attribute__((aligned(128))) const RotOffTable g_rot_off_table = make_rot_off_table(4 * BR_DW);
__device__ __attribute__((aligned(128))) const RotOffTable g_rot_off_table_tiled = make_rot_off_table(4 * BR_DW_TILED);

constexpr int OR_NV = OR_ROWS * (OR_DW / 2);   // 155 dwordx2 vectors of a centroid patch
constexpr int OR_WT = 192;                     // weight entries per byte alignment: one per vector, padded to 3 x 64 lanes
constexpr int OR_WTD = 2 * OR_WT + 1;          // DiscWeightDwTable entries per byte alignment: a zero, then one per patch dword

// The disc weights of orient_rbrief_kernel's s_w as a compile-time table: entry (sh, t) = weights of patch vector t (row
// t / 5, dword pair t % 5) for a patch whose first column sits sh bytes into its first dword: .x/.y = (dx + 15) inside
// the disc else 0 (u8 x 4) of the two dwords, .z/.w = 1 inside the disc else 0.
template <int ALIGN>
struct DiscWeightTable {
  uint32_t v[ALIGN * OR_WT * 4];
};
template <int ALIGN>
constexpr DiscWeightTable<ALIGN> make_disc_weight_table() {
  constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
  DiscWeightTable<ALIGN> r{};
  for (int e = 0; e < ALIGN * OR_WT; ++e) {
    const int sh = e / OR_WT, t = e - sh * OR_WT;
    if (t >= OR_NV) continue;
    const int row = t / (OR_DW / 2), c = t - row * (OR_DW / 2);
    const int dy = row - OR_R, um = umax[dy < 0 ? -dy : dy];
    for (int d = 0; d < 2; ++d)
      for (int b = 0; b < 4; ++b) {
        const int dx = 4 * (2 * c + d) + b - sh - OR_R;
        if (dx >= -um && dx <= um) {
          r.v[4 * e + d] |= (uint32_t)(dx + OR_R) << (8 * b);
          r.v[4 * e + 2 + d] |= 1u << (8 * b);
        }
      }
  }
  return r;
}
__device__ __attribute__((aligned(128))) const DiscWeightTable<4> g_disc_weight_table = make_disc_weight_table<4>();

// The tiled form's disc weights, per dword instead of per dword pair (12 KB of LDS instead of the 24 KB of
// DiscWeightTable<8>): entry (a, j), j >= 1 = {(dx + 15) inside the disc else 0, 1 inside else 0} (u8 x 4) of dword j - 1 of
// the patch's rows laid end to end (10 dwords each), for a patch whose first column sits a bytes into its first dword;
// entry (a, 0) and those past the last row are 0.  A patch that starts sh = 4 s + a bytes before its first column
// weighs its dword d with entry (a, d + 1 - s), so vector t (dwords 2t, 2t + 1) reads entries 2t + 1 - s and 2t + 2 - s.
// For s = 1 and t at a row start the first of them is the previous row's last dword (or entry 0): dx >= 18 there, 0 as
// well.  Vectors t >= 155 (padding lanes) read entries past the last row.
struct DiscWeightDwTable {
  uint32_t v[4 * OR_WTD * 2];
};
constexpr DiscWeightDwTable make_disc_weight_dw_table() {
  constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
  DiscWeightDwTable r{};
  for (int e = 0; e < 4 * OR_WTD; ++e) {
    const int a = e / OR_WTD, d = e - a * OR_WTD - 1;
    if (d < 0 || d >= OR_ROWS * OR_DW) continue;
    const int row = d / OR_DW, col = d - row * OR_DW;
    const int dy = row - OR_R, um = umax[dy < 0 ? -dy : dy];
    for (int b = 0; b < 4; ++b) {
      const int dx = 4 * col + b - a - OR_R;
      if (dx >= -um && dx <= um) {
        r.v[2 * e] |= (uint32_t)(dx + OR_R) << (8 * b);
        r.v[2 * e + 1] |= 1u << (8 * b);
      }
    }
  }
  return r;
}
__device__ __attribute__((aligned(128))) const DiscWeightDwTable g_disc_weight_dw_table = make_disc_weight_dw_table();
constexpr bool disc_weight_dw_table_matches() {   // the same weights as the per-pair table of all 8 alignments, every vector
  constexpr DiscWeightTable<8> pair = make_disc_weight_table<8>();
  constexpr DiscWeightDwTable dw = make_disc_weight_dw_table();
  for (int sh = 0; sh < 8; ++sh)
    for (int t = 0; t < OR_WT; ++t) {
      const int e = (sh & 3) * OR_WTD + 2 * t + 1 - (sh >> 2);
      const uint32_t* p = pair.v + 4 * (sh * OR_WT + t);
      if (dw.v[2 * e] != p[0] || dw.v[2 * e + 2] != p[1] || dw.v[2 * e + 1] != p[2] || dw.v[2 * e + 3] != p[3]) return false;
    }
  return true;
}
static_assert(disc_weight_dw_table_matches(), "DiscWeightDwTable must weigh every vector as DiscWeightTable<8>");

// What orient_rbrief_kernel takes from the plane layout.  Row-major planes: patch rows start on the dword boundary below
// x - radius (4 alignments; EXACT: at x - radius itself).  Block-tiled planes: on the 8-byte boundary below it (8
// alignments), so the descriptor patch needs 44 of 48 bytes (12 dwords) per row; the centroid patch's 38 still fit its 40.
template <bool TILED, bool EXACT = false> struct OrGeom {
  static constexpr int ALIGN = 4, BR_DW = ::BR_DW;
  static constexpr int WT_VEC4 = ALIGN * OR_WT;   // uint4 entries of s_w (DiscWeightTable<4>)
  // GRP: centroid patches of this many keypoints are in flight together.  BLUR_BUF: descriptor patch buffers per wave, 1 or 2.
  static constexpr int GRP = 4, BLUR_BUF = 2;
  static constexpr bool BINS_AFTER_PHASE_A = false;
  typedef PatchRegs<OR_R, OR_DW, EXACT> Disc;
  typedef PatchRegs<BR_R, BR_DW, EXACT> Brief;
  static constexpr const uint32_t* WEIGHT_TABLE = g_disc_weight_table.v;   // s_w is a copy of it
  static constexpr const uint32_t* ROT_TABLE = g_rot_off_table.v;
  // the weights of the lane's vector lane + 64 u of a patch that starts sh bytes before its first column:
  // .x/.y = (dx + 15) inside the disc else 0 (u8 x 4) of the two dwords, .z/.w = 1 inside the disc else 0
  static __device__ __forceinline__ uint4 disc_weights(const uint4* s_w, int sh, int lane, int u) {
    return s_w[sh * OR_WT + lane + 64 * u];
  }
};
template <bool EXACT> struct OrGeom<true, EXACT> {
  static_assert(!EXACT, "tiled planes are always read from aligned starts");
  static constexpr int ALIGN = 8, BR_DW = BR_DW_TILED;
  static constexpr int WT_VEC4 = 4 * OR_WTD * 2 / 4;   // uint4 entries of s_w (DiscWeightDwTable)
  // 7 waves per SIMD: <= 72 VGPRs (phase A keeps 2 centroid patches in flight, not 4; the bin directions are loaded after
  // phase A's patches, 8 registers fewer while they are in flight) and <= 23,405 B of LDS (the weights per dword; ONE
  // descriptor patch buffer per wave -- the ballots of keypoint k have consumed its patch bytes before the patch of k + 1
  // is stored).  tests/test_orient_resources.py holds these figures.
  static constexpr int GRP = 2, BLUR_BUF = 1;
  static constexpr bool BINS_AFTER_PHASE_A = true;
  typedef TiledPatchRegs<OR_R, OR_DW> Disc;
  typedef TiledPatchRegs<BR_R, BR_DW> Brief;
  static constexpr const uint32_t* WEIGHT_TABLE = g_disc_weight_dw_table.v;   // s_w is a copy of it
  static constexpr const uint32_t* ROT_TABLE = g_rot_off_table_tiled.v;
  // the same uint4 from the per-dword table: {moment, count} of the vector's two dwords are entries 2t + 1 - s, 2t + 2 - s
  static __device__ __forceinline__ uint4 disc_weights(const uint4* s_w, int sh, int lane, int u) {
    const uint2* wd = reinterpret_cast<const uint2*>(s_w) + (sh & 3) * OR_WTD + 1 - (sh >> 2) + 2 * lane;
    const uint2 w0 = wd[128 * u], w1 = wd[128 * u + 1];
    return make_uint4(w0.x, w1.x, w0.y, w1.y);
  }
};
static_assert(2 * OR_R + 1 + 7 <= 4 * OR_DW && 2 * BR_R + 1 + 7 <= 4 * BR_DW_TILED, "tiled patch rows: 8-byte aligned starts");
static_assert(sizeof(DiscWeightDwTable) == 16 * OrGeom<true>::WT_VEC4, "LDS copy of the tiled weights: whole uint4");

// One workgroup per image: the image's keypoints counting-sorted by 64 x 64-pixel cell (cells in raster order; inside a
// cell as the atomics fall -- a schedule, not a result).  order [n_img][max_kp]; slots from the image's count on map to
// themselves.
constexpr int OO_CELL = 64, OO_MAX_CELLS = 1024;
__global__ __launch_bounds__(256) void orient_order_kernel(const uint32_t* __restrict__ kp_keys, const int* __restrict__ kp_count,
                                                           int max_kp, int W, int cw, int n_cells, int* __restrict__ order) {
  __shared__ int s_cnt[OO_MAX_CELLS];
  __shared__ int s_wave[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int cnt = clampi(kp_count[n], 0, max_kp);   // a negative count is an empty list: the identity starts at slot 0
  const uint32_t* keys = kp_keys + (size_t)n * max_kp;
  int* ord = order + (size_t)n * max_kp;
  for (int r = tid; r < n_cells; r += 256) s_cnt[r] = 0;
  __syncthreads();
  for (int j = tid; j < cnt; j += 256) {
    const uint32_t pos = keys[j] & VUS_KEY_POS_MASK;
    const int y = (int)(pos / (uint32_t)W), x = (int)(pos - (uint32_t)y * (uint32_t)W);
    atomicAdd(&s_cnt[(y / OO_CELL) * cw + (x / OO_CELL)], 1);
  }
  __syncthreads();
  int c[4], sum = 0;      // exclusive scan of the <= 1024 counts: four consecutive cells per thread
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    c[q] = 4 * tid + q < n_cells ? s_cnt[4 * tid + q] : 0;
    sum += c[q];
  }
  int incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d);
    if ((tid & 63) >= d) incl += o;
  }
  if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
  __syncthreads();
  int base = incl - sum;
  for (int w = 0; w < (tid >> 6); ++w) base += s_wave[w];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (4 * tid + q < n_cells) {
      s_cnt[4 * tid + q] = base;   // becomes the cell's fill cursor
      base += c[q];
    }
  __syncthreads();
  for (int j = tid; j < cnt; j += 256) {
    const uint32_t pos = keys[j] & VUS_KEY_POS_MASK;
    const int y = (int)(pos / (uint32_t)W), x = (int)(pos - (uint32_t)y * (uint32_t)W);
    ord[atomicAdd(&s_cnt[(y / OO_CELL) * cw + (x / OO_CELL)], 1)] = j;
  }
  for (int j = cnt + tid; j < max_kp; j += 256) ord[j] = j;
}

}  // namespace

extern "C" int vus_orient_order(const uint32_t* kp_keys, const int* kp_count, int n_img, int max_kp, int H, int W, int* order,
                                void* stream) {
  VUS_REQUIRE(kp_keys && kp_count && order, "null buffer");
  VUS_REQUIRE(n_img >= 0 && max_kp >= 1 && H >= 1 && W >= 1, "n_img=%d max_kp=%d H=%d W=%d", n_img, max_kp, H, W);
  if (n_img == 0) return VUS_OK;
  // cells of 64 x 64 pixels; an image with more than 1024 of them is refused (include/vus.h: the caller then uses
  // vus_orient_rbrief, which needs no order)
  int cw = (W + OO_CELL - 1) / OO_CELL, ch = (H + OO_CELL - 1) / OO_CELL;
  VUS_REQUIRE((long long)cw * ch <= OO_MAX_CELLS, "image of %d x %d pixels has more than %d cells of %d x %d", W, H, OO_MAX_CELLS,
              OO_CELL, OO_CELL);
  orient_order_kernel<<<n_img, 256, 0, vus::as_stream(stream)>>>(kp_keys, kp_count, max_kp, W, cw, cw * ch, order);
  VUS_CHECK_LAUNCH("orient_order");
  return VUS_OK;
}

namespace {

// One wave = eight consecutive keypoints of one image, in two phases.
//  A. orientation of all eight: the 31-row image patches arrive in registers (3 dwordx2 per lane and keypoint, those of
//     GRP keypoints in flight) and are multiplied right there with the disc weights (v_dot4_u32_u8; the weights of a lane's two dwords
//     are ONE LDS read): no LDS round trip for the patch.  Per-lane partial moments of the eight keypoints
//     -> reduce-scatter (fold32 .. allsum8 above) -> lane 8g + j holds m10 / m01 of keypoint g and ranks bins 4j .. 4j+3.
//  B. descriptors, keypoint by keypoint: the 37-row patch of the smoothed image goes through LDS (BLUR_BUF buffers; the
//     next keypoint's rows and its bin's test offsets are in flight meanwhile), 8 byte reads + 4 compares per lane; the
//     ballots are written into lanes 4k + w of one register pair, so the eight descriptors leave in ONE 256-byte store.
// Its predecessor, one keypoint at a time: 232 vector instructions per keypoint (2.67 ms per 1000 stereo frames).
// ORDERED: slot s of an image is served with keypoint order[s] (vus_orient_order: the image's keypoints grouped by 64 x 64
// cell, the unused slots mapped to themselves), so that the eight keypoints of a wave and the 32 of a workgroup are
// neighbours and their patch rows share lines in flight; the outputs go to the keypoint's own index.  A schedule only.
// TILED: img and blur are block-tiled planes (include/vus_tiled.h, pitch = W).  OrGeom carries every difference: the
// patch loaders, the weight and test-offset tables, the patches in flight.  Phase B's LDS patch stays row-major
// (48-byte rows), so the ballots are those of the plain form.
template <bool EXACT, bool ORDERED, bool TILED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TILED ? VUS_OR_WPE_TILED : VUS_OR_WPE, 8))) void orient_rbrief_kernel(
    const uint8_t* __restrict__ img, const uint8_t* __restrict__ blur, int H, int W, int pitch,
    const uint32_t* __restrict__ kp_keys, const int* __restrict__ kp_count, int max_kp, const int* __restrict__ order,
    uint64_t* __restrict__ desc_out, uint8_t* __restrict__ angle_out, int n_img, int chunks_per_img) {
  typedef OrGeom<TILED, EXACT> G;
  __shared__ uint4 s_w[G::WT_VEC4];   // the disc weights for every byte alignment of a centroid patch (G::disc_weights)
  __shared__ __attribute__((aligned(8))) uint32_t s_blur[4][G::BLUR_BUF][BR_ROWS * G::BR_DW];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware block -> (image, chunk) map: workgroups are dealt round-robin over the 8 XCDs, so all
  // chunks of one image go to blocks with equal (blockIdx % 8): the image's two 0.9 MB planes then
  // stay in ONE XCD's 4 MiB L2 while its 2000 patches are gathered (placement affects speed only).
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int n = (slot / chunks_per_img) * 8 + xcd;
  const int chunk = slot - (slot / chunks_per_img) * chunks_per_img;
  if (n >= n_img) return;
  {   // the disc weights: a compile-time table, copied (deriving them per workgroup cost ~19 vector instructions per keypoint)
    const uint4* wt = reinterpret_cast<const uint4*>(G::WEIGHT_TABLE);
#pragma unroll
    for (int i = 0; i < (G::WT_VEC4 + 255) / 256; ++i)
      if (G::WT_VEC4 % 256 == 0 || threadIdx.x + 256 * i < G::WT_VEC4) s_w[threadIdx.x + 256 * i] = wt[threadIdx.x + 256 * i];
  }
  const uint8_t* im = img + (size_t)n * H * pitch;
  const uint8_t* bl = blur + (size_t)n * H * W;   // TILED: both planes have H * W bytes per image
  const int base_i = (chunk * 4 + wave) * OR_KP_PER_WAVE;       // this wave's keypoints: base_i .. base_i + 7
  const int n_live = clampi(min(kp_count[n], max_kp) - base_i, 0, OR_KP_PER_WAVE);
  int my_y = 0, my_x = 0;                                         // lane k < 8: position of keypoint k
  int my_idx = base_i + lane;                                     // ... and its index in the image's list
  if (ORDERED && lane < OR_KP_PER_WAVE && base_i + lane < max_kp) my_idx = order[(size_t)n * max_kp + base_i + lane];
  if (lane < n_live) {
    const uint32_t pos = kp_keys[(size_t)n * max_kp + my_idx] & VUS_KEY_POS_MASK;
    my_y = (int)(pos / (uint32_t)W);
    my_x = (int)(pos - (uint32_t)my_y * (uint32_t)W);
  }
  // the directions of the bins this lane ranks after phase A: 4 (lane & 7) + q.  Loaded here, or behind phase A's patches
  // (G::BINS_AFTER_PHASE_A, a register-pressure decision)
  int bin_cos[4], bin_sin[4];
  if constexpr (!G::BINS_AFTER_PHASE_A) load_bin_directions(VUS_ANGLE_COS, VUS_ANGLE_SIN, lane, bin_cos, bin_sin);
  constexpr int GRP = G::GRP;
  typename G::Disc pr[GRP];
  typename G::Brief pb;
#pragma unroll
  for (int kk = 0; kk < GRP; ++kk) pr[kk].init(pitch, lane);
  pb.init(W, lane);
  int mom_dy[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) mom_dy[u] = min(lane + 64 * u, OR_NV - 1) / (OR_DW / 2) - OR_R;
  __syncthreads();   // the weight table is complete (the only workgroup-level synchronisation of the kernel)
  if (n_live == 0) {   // wave-uniform: nothing but defined contents for the unused slots
    if (lane < 4 * OR_KP_PER_WAVE && base_i + (lane >> 2) < max_kp) desc_out[((size_t)n * max_kp + base_i) * 4 + lane] = 0;
    if (lane < OR_KP_PER_WAVE && base_i + lane < max_kp) angle_out[(size_t)n * max_kp + base_i + lane] = 0;
    return;
  }

  // ---- phase A: centroid moments of the eight keypoints, GRP at a time
  int pa[8], pq[8];   // per-lane partials of m10 and m01
#pragma unroll
  for (int g = 0; g < 8 / GRP; ++g) {
#pragma unroll
    for (int kk = 0; kk < GRP; ++kk) {
      const int k = GRP * g + kk;
      if (k < n_live) pr[kk].load(im, H, W, pitch, __builtin_amdgcn_readlane(my_y, k), __builtin_amdgcn_readlane(my_x, k), lane);
    }
    if (g == 8 / GRP - 1)   // the first descriptor patch joins the queue behind the last centroid patches
      pb.load(bl, H, W, W, __builtin_amdgcn_readlane(my_y, 0), __builtin_amdgcn_readlane(my_x, 0), lane);
#pragma unroll
    for (int kk = 0; kk < GRP; ++kk) {
      const int k = GRP * g + kk;
      pa[k] = 0;
      pq[k] = 0;
      if (k < n_live) {
        const int sh = EXACT ? 0 : (__builtin_amdgcn_readlane(my_x, k) - OR_R) & (G::ALIGN - 1);
        uint32_t sx = 0;
        int si = 0, sy = 0;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const uint4 w = G::disc_weights(s_w, sh, lane, u);
          sx = __builtin_amdgcn_udot4(pr[kk].v[u][0], w.x, sx, false);
          sx = __builtin_amdgcn_udot4(pr[kk].v[u][1], w.y, sx, false);
          uint32_t rs = __builtin_amdgcn_udot4(pr[kk].v[u][0], w.z, 0u, false);
          rs = __builtin_amdgcn_udot4(pr[kk].v[u][1], w.w, rs, false);
          si += (int)rs;
          sy += mom_dy[u] * (int)rs;
        }
        pa[k] = (int)sx - OR_R * si;   // sum dx I over this lane's pixels
        pq[k] = sy;                    // sum dy I
      }
    }
  }
  if constexpr (G::BINS_AFTER_PHASE_A) load_bin_directions(VUS_ANGLE_COS, VUS_ANGLE_SIN, lane, bin_cos, bin_sin);
  // reduce-scatter: afterwards the lanes of group g = lane / 8 hold the moments of keypoint g
  int m10, m01;
  {
    const bool up8 = (lane & 8) != 0;
    int c[4], d[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = fold32(pa[j], pa[j + 4]);        // lanes < 32: keypoint j, else j + 4
#pragma unroll
    for (int j = 0; j < 2; ++j) d[j] = fold16(c[j], c[j + 2]);          // row r: keypoint j + 2 r
    m10 = allsum8(fold8(d[0], d[1], up8));                              // group g: keypoint g
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = fold32(pq[j], pq[j + 4]);
#pragma unroll
    for (int j = 0; j < 2; ++j) d[j] = fold16(c[j], c[j + 2]);
    m01 = allsum8(fold8(d[0], d[1], up8));
  }
  // nearest bin direction = largest projection, first maximum wins (integer, exact):
  // |prj| < 2^38, so (prj << 5) | (31 - bin) orders by projection, then by lowest bin, in one 64-bit max
  int my_bin;
  {
    long long best = (long long)(-0x7FFFFFFFFFFFFFFFll - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int bq = 4 * (lane & 7) + q;
      long long key = ((long long)m10 * bin_cos[q] + (long long)m01 * bin_sin[q]) * 32 + (31 - bq);
      if (bq >= VUS_N_ANGLE_BINS) key = (long long)(-0x7FFFFFFFFFFFFFFFll - 1);
      best = key > best ? key : best;
    }
    best = allmax8_i64(best);
    my_bin = 31 - (int)(best & 31);   // a keypoint that is not live has zero moments: bin 0
  }
  {
    const int j_ang = ORDERED ? __shfl(my_idx, lane >> 3) : base_i + (lane >> 3);
    if ((lane & 7) == 0 && base_i + (lane >> 3) < max_kp) angle_out[(size_t)n * max_kp + j_ang] = (uint8_t)my_bin;
  }

  // ---- phase B: the descriptors
  uint32_t wlo = 0, whi = 0;   // lane 4k + w: word w of keypoint k
  const uint4* rot = reinterpret_cast<const uint4*>(G::ROT_TABLE) + lane;
  uint4 to = rot[__builtin_amdgcn_readlane(my_bin, 0) * 64];
  for (int k = 0; k < n_live; ++k) {   // scalar loop
    uint32_t* patch = s_blur[wave][k & (G::BLUR_BUF - 1)];
    pb.store(patch, lane);
    const uint4 cto = to;
    const int cx = __builtin_amdgcn_readlane(my_x, k);
    if (k + 1 < n_live) {
      pb.load(bl, H, W, W, __builtin_amdgcn_readlane(my_y, k + 1), __builtin_amdgcn_readlane(my_x, k + 1), lane);
      to = rot[__builtin_amdgcn_readlane(my_bin, 8 * (k + 1)) * 64];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // this wave's LDS operations execute in order
    const int sh_blur = EXACT ? 0 : (cx - BR_R) & (G::ALIGN - 1);   // patch column of x - radius
    const uint8_t* c = reinterpret_cast<const uint8_t*>(patch) + BR_R * (4 * G::BR_DW) + BR_R + sh_blur;   // the keypoint inside the patch
    const uint32_t tw[4] = {cto.x, cto.y, cto.z, cto.w};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int a = c[(int16_t)(tw[w] & 0xFFFFu)];
      const int b = c[(int16_t)(tw[w] >> 16)];
      const uint64_t word = __ballot(a < b);  // lane l supplies bit l of word w
      wlo = writelane_u32(wlo, (uint32_t)word, 4 * k + w);
      whi = writelane_u32(whi, (uint32_t)(word >> 32), 4 * k + w);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  const int j_desc = ORDERED ? __shfl(my_idx, lane >> 2) : 0;   // keypoint k's index lives in lane k; lanes 4k .. 4k+3 store its words
  if (lane < 4 * OR_KP_PER_WAVE && base_i + (lane >> 2) < max_kp)
    desc_out[ORDERED ? ((size_t)n * max_kp + j_desc) * 4 + (lane & 3) : ((size_t)n * max_kp + base_i) * 4 + lane] =
        ((uint64_t)whi << 32) | wlo;
}

}  // namespace

// The launch behind the three vus_orient_rbrief* entry points.  tiled: block-tiled planes, pitch == W.
static int orient_launch(bool tiled, const uint8_t* img, const uint8_t* blur, int n_img, int H, int W, int pitch,
                         const uint32_t* kp_keys, const int* kp_count, int max_kp, const int* order, uint64_t* desc_out,
                         uint8_t* angle_out, void* stream) {
  if (int rc = check_image_args(img, n_img, H, W, pitch)) return rc;
  if (tiled)
    if (int rc = check_tiled_args(img, blur, H, W)) return rc;
  VUS_REQUIRE(blur && kp_keys && kp_count && desc_out && angle_out, "null buffer");
  VUS_REQUIRE(max_kp >= 1, "max_kp=%d", max_kp);
  if (n_img == 0) return VUS_OK;
  const int chunks = (max_kp + 4 * OR_KP_PER_WAVE - 1) / (4 * OR_KP_PER_WAVE);
  const long long blocks = (long long)((n_img + 7) / 8) * 8 * chunks;
  VUS_REQUIRE(blocks < (1ll << 31), "too many workgroups (%lld)", blocks);
  // rows of both planes on dword boundaries -> aligned patch loads; otherwise exact-start (unaligned) loads (row-major
  // planes only: the tiled ones are 16-byte aligned throughout)
  const bool aligned = ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(blur) | (uintptr_t)pitch |
                         (uintptr_t)W | ((uintptr_t)H * (uintptr_t)pitch)) & 3u) == 0;
  auto launch = [&](auto exact, auto ordered, auto tiled_planes) {
    orient_rbrief_kernel<decltype(exact)::value, decltype(ordered)::value, decltype(tiled_planes)::value>
        <<<(unsigned)blocks, 256, 0, vus::as_stream(stream)>>>(img, blur, H, W, pitch, kp_keys, kp_count, max_kp, order, desc_out,
                                                               angle_out, n_img, chunks);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (!tiled && aligned) order ? launch(no, yes, no) : launch(no, no, no);
  else if (!tiled) order ? launch(yes, yes, no) : launch(yes, no, no);
  else order ? launch(no, yes, yes) : launch(no, no, yes);
  VUS_CHECK_LAUNCH(tiled ? "orient_rbrief_tiled" : "orient_rbrief");
  return VUS_OK;
}

extern "C" int vus_orient_rbrief(const uint8_t* img, const uint8_t* blur, int n_img, int H, int W, int pitch,
                                 const uint32_t* kp_keys, const int* kp_count, int max_kp,
                                 uint64_t* desc_out, uint8_t* angle_out, void* stream) {
  return orient_launch(false, img, blur, n_img, H, W, pitch, kp_keys, kp_count, max_kp, nullptr, desc_out, angle_out, stream);
}

extern "C" int vus_orient_rbrief_ordered(const uint8_t* img, const uint8_t* blur, int n_img, int H, int W, int pitch,
                                         const uint32_t* kp_keys, const int* kp_count, int max_kp, const int* order,
                                         uint64_t* desc_out, uint8_t* angle_out, void* stream) {
  VUS_REQUIRE(order != nullptr, "null buffer");
  return orient_launch(false, img, blur, n_img, H, W, pitch, kp_keys, kp_count, max_kp, order, desc_out, angle_out, stream);
}

extern "C" int vus_orient_rbrief_tiled(const uint8_t* img_tiled, const uint8_t* blur_tiled, int n_img, int H, int W,
                                       const uint32_t* kp_keys, const int* kp_count, int max_kp, const int* order,
                                       uint64_t* desc_out, uint8_t* angle_out, void* stream) {
  return orient_launch(true, img_tiled, blur_tiled, n_img, H, W, W, kp_keys, kp_count, max_kp, order, desc_out, angle_out, stream);
}
