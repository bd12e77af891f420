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
#ifndef VUS_OR_WPE_TILED_MAX
#define VUS_OR_WPE_TILED_MAX 7   // ... and not more: with the folded weight table 8 fit (63 VGPRs, 18,720 B of LDS) and are slower
#endif                           // (profiles/orient_lds_r10.md)
constexpr int OR_R = 15;                    // disc radius
constexpr int OR_ROWS = 2 * OR_R + 1;       // 31
constexpr int OR_DW = 10;                   // 36 bytes cover x-15..x+15 from an aligned start; whole dwordx2 are loaded
constexpr int BR_R = VUS_RBRIEF_REACH;      // 18
constexpr int BR_ROWS = 2 * BR_R + 1;       // 37
constexpr int BR_DW = 10;                   // 40 bytes cover x-18..x+18 from an aligned start
constexpr int BR_DW_TILED = 20;             // block-tiled planes: 80-byte rows in LDS, three 16-byte block rows, a dword of the fourth (OrGeom) and 28 bytes of pad
constexpr int OR_PC = 3;                    // block-tiled planes: 31 + 15 bytes of a centroid patch row lie in three block rows
constexpr int OR_NP = OR_ROWS * OR_PC;      // 93 pieces of a centroid patch
constexpr int OR_KP_PER_WAVE = 8;           // keypoints of one wave; the reduce-scatter and the one-store epilogue are written for 8
constexpr int OR_WFOLD = OR_R + 1;          // block-tiled planes: rows r and 30 - r weigh alike, the weight table holds 16 rows
constexpr int OR_WROW = 4 * OR_PC + 1;      // ... of 13 eight-byte entries: 12 dwords and a pad, an ODD stride (DiscWeightDwTable)

// Load a (2*RADIUS+1) x (4*DW)-byte patch around (x, y) into registers: every lane issues all of
// its loads back to back (one memory round trip), the caller stores them to LDS afterwards.
// A lane moves two dwords per load (dwordx2 at dword alignment): the texture path's cost is per instruction, not per
// byte.  Measured and not kept, ms per 1000 frames against the 2.82 of 6 dwordx2 per keypoint: 11 dword loads: 3.19;
// 4 dwordx4 of 48-byte rows: 3.04 (dword-aligned, so they straddle 16-byte boundaries).  On block-tiled planes, naturally
// aligned dwordx4 of whole block rows (below), ms per 1000 stereo frames against the 1.71 of 7 dwordx2 per keypoint: 3.75
// loads with 9 % more bytes (kept): 1.58; 3.75 loads with 13 % more bytes: 1.61; 4.5 loads with 28 % more bytes: 1.85 --
// there the cost followed the instructions AND the bytes, about 0.08 ms per load and keypoint and 0.4 ms per 1000 bytes and
// keypoint (profiles/orient_block_rows_r08.md).  The L1's ACCESSES are a small part of the per-byte share: with the same
// bytes in the same loads, dealt so that an even lane and its neighbour read 32 contiguous bytes (PieceRC below), the
// accesses fall from 216.9 to 128.3 per keypoint and the time from 1.569 to 1.499 ms, about 0.08 ms per 100 accesses and
// keypoint -- 1000 bytes are 62.5 accesses of 16, 0.05 of their 0.4 ms.  The rest follows the bytes themselves
// (profiles/orient_lane_dealing_r09.md).
// With the gather cut that far the tiled kernel was bound by LDS, not by its loads: the LDS array was busy for 92 % of the
// launch (210 cycles per keypoint, 147 of them bank conflicts), 94 of the cycles in the weight reads of phase A alone and
// 74 in the byte reads of phase B.  The weight table in rows of 13 entries, folded (DiscWeightDwTable), and the descriptor
// patch in rows of 80 bytes (TiledBriefRegs) leave 119 cycles, 60 % of a shorter launch: 1.494 -> 1.375 ms per 1000 stereo
// frames, nearly all of it from the weights; the waves now wait on their patch loads again.  tools/lds_bank_model.py
// states the bank rules and gives the conflicts of each layout to within 1 % (profiles/orient_lds_r10.md).
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

// Patches from a block-tiled plane (include/vus_tiled.h; W % 16 == 0, H % 8 == 0).  A lane's vector is one whole
// 16-byte block row (dwordx4, naturally aligned: it never straddles a block row), and the patch starts at the 16-byte
// boundary xa below x - RADIUS.  Piece (r, c) -- pixels (y0 + r, xa + 16 c .. + 15) -- sits at
//   tiled(y0 & ~7, xa)  +  16 (y0 & 7)  +  16 r + 128 c  +  (p >> 3) (8 W - 128),   p = (y0 & 7) + r
// -- the first two terms wave-uniform per keypoint, 16 r + 128 c a per-lane constant.  Keypoints whose window leaves the
// image take the replicate-clamped byte path.
__device__ __forceinline__ uint4 tiled_piece_clamped(const uint8_t* __restrict__ src, int H, int W, int gy, int gx) {
  gy = clampi(gy, 0, H - 1);
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w[j] = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) w[j] |= (uint32_t)src[vus_tiled_offset(gy, clampi(gx + 4 * j + b, 0, W - 1), W)] << (8 * b);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The DEALING of a patch's pieces to the lanes of its wave-loads: slot -> (r, c), the one definition that the loaders'
// fast and clamped paths, the LDS stores and the weights follow.  The eight 16-byte rows of a block are ONE 128-byte line,
// so neighbouring lanes take neighbouring ROWS of one piece column: a lane group then asks for contiguous bytes of one
// line.  With the piece column fastest (slot = 3 r + c) neighbouring lanes asked three lines, 128 bytes apart, for 16
// bytes each, and the L1 saw one access per piece: 216.9 per keypoint against 128.3 now, for the same bytes and the same
// load instructions.  The counts fit a texture path that merges the dwordx4 of an even lane and its neighbour when they
// are 32 contiguous bytes, and nothing wider (profiles/orient_lane_dealing_r09.md: 1.569 -> 1.499 ms per 1000 stereo frames).
struct PieceRC {
  int r, c;   // r >= the patch's rows: an idle slot
};
constexpr int BR_PC = 3;                    // whole pieces per row of the descriptor patch (TiledBriefRegs)
// centroid patch, 93 slots: rows fastest, q = 31 c + r
__host__ __device__ constexpr PieceRC disc_piece(int q) {
  const int c = (q >= OR_ROWS ? 1 : 0) + (q >= 2 * OR_ROWS ? 1 : 0);
  return {q - OR_ROWS * c, c};
}
// ... and the first of the four weight entries of piece (r, c), before the patch's alignment moves it (DiscWeightDwTable)
__host__ __device__ constexpr int disc_weight_entry(int r, int c) { return OR_WROW * (r < OR_ROWS - 1 - r ? r : OR_ROWS - 1 - r) + 4 * c; }
// descriptor patch: four rows of one column, then the next column's -- t = 12 g + 4 c + j holds row 4 g + j; 120 slots, the
// rows 37 .. 39 of the last group idle.  Its pieces go on to LDS rows of 80 bytes (64 when this was measured; the model
// gives both pitches the same 29 cycles), where a ds_write_b128 serves eight neighbouring lanes at a time on 32 banks: four
// rows of two columns meet two to a bank, at the instruction's own cost.
// Rows fastest (t = 37 c + r) meet four to a bank and lost more there than the gather gained: 1.609 ms against the 1.527
// of the piece column fastest and the 1.499 of this form, the centroid patch as above in all three.
constexpr int BR_GROUP_ROWS = 4;            // rows of a group (tools/lds_bank_model.py reads the dealing from these constants)
constexpr int BR_SLOTS = BR_GROUP_ROWS * BR_PC * ((BR_ROWS + BR_GROUP_ROWS - 1) / BR_GROUP_ROWS);
static_assert(BR_GROUP_ROWS == 4 && BR_GROUP_ROWS * BR_PC == 12, "brief_piece divides by 12 and by 4 with shifts");
__host__ __device__ constexpr PieceRC brief_piece(int t) {
  const int g = (t * 171) >> 11, w = t - 12 * g;   // t / 12 for t < 128
  return {4 * g + (w & 3), w >> 2};
}
template <int ROWS, int PC, int SLOTS, PieceRC (*PIECE)(int)>
constexpr bool dealing_is_a_permutation() {   // every piece in exactly one slot, every other slot idle
  bool seen[ROWS * PC] = {};
  int n = 0;
  for (int s = 0; s < SLOTS; ++s) {
    const PieceRC p = PIECE(s);
    if (p.r < 0 || p.c < 0 || p.c >= PC) return false;
    if (p.r >= ROWS) continue;
    if (seen[p.r * PC + p.c]) return false;
    seen[p.r * PC + p.c] = true;
    ++n;
  }
  return n == ROWS * PC;
}
static_assert(dealing_is_a_permutation<OR_ROWS, OR_PC, OR_NP, disc_piece>(), "centroid patch: 31 x 3 pieces, one slot each");
static_assert(dealing_is_a_permutation<BR_ROWS, BR_PC, BR_SLOTS, brief_piece>(), "descriptor patch: 37 x 3 pieces, one slot each");
static_assert(BR_SLOTS <= 128, "descriptor patch: two wave-loads");

// The centroid patches of TWO keypoints, 93 pieces each, dealt to the lanes back to back: slot p = lane + 64 u
// (u < 3) belongs to keypoint p / 93 and holds piece disc_piece(p % 93) of its patch.  Wave-load 0 is all first keypoint,
// wave-load 2 all second, wave-load 1 changes over at lane SPLIT: 1.5 loads per keypoint.  Slots 186 .. 191, and the
// second keypoint's when it is not live, are not read and hold 0.
struct TiledDiscPair {
  static constexpr int ITERS = (2 * OR_NP + 63) / 64;   // 3
  static constexpr int SPLIT = OR_NP - 64;              // 29
  static_assert(ITERS == 3 && SPLIT > 0 && SPLIT < 64, "wave-load 1 is the only mixed one");
  // pk, a lane's piece (r, c) in one register: bits 0 .. 9 its byte offset 16 r + 128 c, bits 10 .. 19 the entry of its
  // weights, disc_weight_entry(r, c) (OrGeom<true>::pair_moments), bits 20 .. 25 its row, with room for (y0 & 7) + r
  static constexpr int PK_OFF_BITS = 10, PK_IDX_SHIFT = 10, PK_IDX_BITS = 10, PK_ROW_SHIFT = 20, PK_ROW_BITS = 6;
  static_assert(16 * (OR_ROWS - 1) + 128 * (OR_PC - 1) < (1 << PK_OFF_BITS) && PK_OFF_BITS <= PK_IDX_SHIFT, "pk: the offset field");
  static_assert(disc_weight_entry(OR_R, OR_PC - 1) < (1 << PK_IDX_BITS) && PK_IDX_SHIFT + PK_IDX_BITS <= PK_ROW_SHIFT, "pk: the weight entry field");
  static_assert(OR_ROWS - 1 + 7 < (1 << PK_ROW_BITS) && PK_ROW_SHIFT + PK_ROW_BITS <= 32, "pk: the row field, nothing above it");
  uint4 v[ITERS];
  uint32_t pk[ITERS];   // this lane's pieces

  static __device__ __forceinline__ int slot_of(int p) { return p >= OR_NP ? p - OR_NP : p; }   // inside its keypoint's patch
  __device__ __forceinline__ void init(int /*pitch*/, int lane) {
#pragma unroll
    for (int u = 0; u < ITERS; ++u) {
      const PieceRC pc = disc_piece(slot_of(min(lane + 64 * u, 2 * OR_NP - 1)));
      const uint32_t r = (uint32_t)pc.r, c = (uint32_t)pc.c;
      pk[u] = r << PK_ROW_SHIFT | (uint32_t)disc_weight_entry(pc.r, pc.c) << PK_IDX_SHIFT | (16u * r + 128u * c);
    }
  }
  __device__ __forceinline__ int row(int u) const { return (int)(pk[u] >> PK_ROW_SHIFT); }
  __device__ __forceinline__ int weight_entry(int u) const { return (int)((pk[u] >> PK_IDX_SHIFT) & ((1u << PK_IDX_BITS) - 1u)); }
  static __device__ __forceinline__ bool inside(int H, int W, int y, int x) {
    const int xa = (x - OR_R) & ~15;
    return y - OR_R >= 0 && y + OR_R < H && xa >= 0 && xa + 16 * OR_PC <= W;
  }
  // (ya, xa): the first keypoint, (yb, xb): the second, read only if b_live (wave-uniform)
  __device__ __forceinline__ void load(const uint8_t* __restrict__ src, int H, int W, int ya, int xa, int yb, int xb, bool b_live,
                                       int lane) {
    const bool second = lane >= SPLIT;   // of wave-load 1
    const bool idle2 = lane >= 2 * OR_NP - 128;
    if (inside(H, W, ya, xa) && (!b_live || inside(H, W, yb, xb))) {   // wave-uniform
      const int y0a = ya - OR_R, y0b = yb - OR_R;
      const uint32_t koa = vus_tiled_offset(y0a & ~7, (xa - OR_R) & ~15, W) + 16u * (uint32_t)(y0a & 7);
      const uint32_t kob = b_live ? vus_tiled_offset(y0b & ~7, (xb - OR_R) & ~15, W) + 16u * (uint32_t)(y0b & 7) : koa;
      const uint32_t ysa = (uint32_t)(y0a & 7) << PK_ROW_SHIFT, ysb = (uint32_t)(y0b & 7) << PK_ROW_SHIFT, ystep = 8u * (uint32_t)W - 128u;
      constexpr int BLK = PK_ROW_SHIFT + 3;                   // (ys + r) >> 3 == (pk + ys) >> BLK: the row field has room for ys + r < 64
      constexpr uint32_t OFF = (1u << PK_OFF_BITS) - 1u;
      v[0] = *reinterpret_cast<const uint4*>(src + koa + (size_t)(((pk[0] + ysa) >> BLK) * ystep + (pk[0] & OFF)));
      v[1] = make_uint4(0u, 0u, 0u, 0u);
      v[2] = make_uint4(0u, 0u, 0u, 0u);
      if (!second || b_live)
        v[1] = *reinterpret_cast<const uint4*>(
            src + (size_t)((second ? kob : koa) + ((pk[1] + (second ? ysb : ysa)) >> BLK) * ystep + (pk[1] & OFF)));
      if (b_live && !idle2)
        v[2] = *reinterpret_cast<const uint4*>(src + kob + (size_t)(((pk[2] + ysb) >> BLK) * ystep + (pk[2] & OFF)));
    } else {        // replicate-clamped, byte by byte (a keypoint of the pair near the image edge)
#pragma unroll
      for (int u = 0; u < ITERS; ++u) {
        const int p = lane + 64 * u;
        const bool sec = p >= OR_NP;
        const PieceRC pc = disc_piece(slot_of(min(p, 2 * OR_NP - 1)));
        const int y = sec ? yb : ya, x = sec ? xb : xa;
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (p < 2 * OR_NP && (!sec || b_live)) v[u] = tiled_piece_clamped(src, H, W, y - OR_R + pc.r, ((x - OR_R) & ~15) + 16 * pc.c);
      }
    }
  }
};

// The 37-row descriptor patch: 37 + a bytes per row from the 16-byte boundary below x - 18, a = (x - 18) & 15.  Three pieces
// per row hold 48 of them (111 pieces, two wave-loads): all of the window for a <= 11.  For a > 11 the window ends 1 .. 4
// bytes into the fourth block row, and ONE dword of that block row is read per patch row (row r in lane r, a third
// wave-load of 148 bytes) -- wave-uniform per keypoint.  Four whole pieces per row (148 pieces, three dwordx4) for every
// keypoint cost 1.85 ms per 1000 stereo frames against the 1.71 of the dwordx2 form, for a > 11 only 1.61, this form 1.58
// (profiles/orient_block_rows_r08.md).  Slot t = lane + 64 u holds piece brief_piece(t), worked out from the lane number where
// it is used: the struct keeps no per-lane constants.
// In LDS the patch has 80-byte rows (BR_DW_TILED), piece (r, c) at 80 r + 16 c, the dword at 80 r + 48; what is not written
// is not read.  The pitch is for the byte reads of the 256 tests, 32 lanes at a time on 32 banks: with 64-byte rows the rows
// r and r + 2 share all their banks and the eight reads took 74 LDS cycles per keypoint, 58 of them conflicts; rows of 20
// dwords spread eight consecutive rows over the banks, 50 cycles (measured: 28 fewer; tests/test_orient_lds_model.py).
struct TiledBriefRegs {
  static constexpr int ROWS = BR_ROWS;
  uint4 v[2];
  uint32_t col;   // a > 11: bytes 48 .. 51 of row `lane`

  static __device__ __forceinline__ bool wide(int x) { return ((x - BR_R) & 15) > 11; }
  // the piece that the lane's slot lane + 64 u is loaded with: an idle slot reads a piece of the last row again (its line is
  // in flight anyway) and is not stored
  static __device__ __forceinline__ PieceRC loaded_piece(int lane, int u) {
    const PieceRC p = brief_piece(min(lane + 64 * u, BR_SLOTS - 1));
    return {min(p.r, ROWS - 1), p.c};
  }
  __device__ __forceinline__ void init(int /*pitch*/, int /*lane*/) { col = 0; }
  __device__ __forceinline__ void load(const uint8_t* __restrict__ src, int H, int W, int /*pitch*/, int y, int x, int lane) {
    const int xa = (x - BR_R) & ~15, y0 = y - BR_R, rc = min(lane, ROWS - 1);
    const bool inside = y0 >= 0 && y + BR_R < H && xa >= 0 && xa + (wide(x) ? 64 : 48) <= W;
    if (inside) {   // wave-uniform
      const uint8_t* base = src + vus_tiled_offset(y0 & ~7, xa, W) + 16 * (y0 & 7);
      const uint32_t ys = (uint32_t)(y0 & 7), ystep = 8u * (uint32_t)W - 128u;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const PieceRC p = loaded_piece(lane, u);
        const uint32_t off = (((uint32_t)p.r + ys) >> 3) * ystep + 16u * (uint32_t)p.r + 128u * (uint32_t)p.c;
        v[u] = *reinterpret_cast<const uint4*>(base + (size_t)off);
      }
      if (wide(x))
        col = *reinterpret_cast<const uint32_t*>(base + (size_t)((((uint32_t)rc + ys) >> 3) * ystep + 16u * (uint32_t)rc + 384u));
    } else {        // replicate-clamped, byte by byte (keypoints near the image edge)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const PieceRC p = loaded_piece(lane, u);
        v[u] = tiled_piece_clamped(src, H, W, y0 + p.r, xa + 16 * p.c);
      }
      if (wide(x)) {
        const int gy = clampi(y0 + rc, 0, H - 1);
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w |= (uint32_t)src[vus_tiled_offset(gy, clampi(xa + 48 + b, 0, W - 1), W)] << (8 * b);
        col = w;
      }
    }
  }
  // x: the keypoint the registers were loaded for
  __device__ __forceinline__ void store(uint32_t* __restrict__ dst, int lane, int x) const {
    uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = lane + 64 * u;
      const PieceRC p = brief_piece(min(t, BR_SLOTS - 1));
      if (t < BR_SLOTS && p.r < ROWS) d[(BR_DW_TILED / 4) * p.r + p.c] = v[u];   // 80 r + 16 c
    }
    if (wide(x) && lane < ROWS) dst[BR_DW_TILED * lane + 12] = col;   // 80 r + 48
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

// The disc weights of orient_rbrief_kernel's s_w as a compile-time table: entry (sh, t) = weights of patch vector t (row
// t / 5, dword pair t % 5) for a patch whose first column sits sh bytes into its first dword: .x/.y = (dx + 15) inside
// the disc else 0 (u8 x 4) of the two dwords, .z/.w = 1 inside the disc else 0.
template <int ALIGN>
struct DiscWeightTable {
  uint32_t v[ALIGN * OR_WT * 4];
};
// {(dx + 15) inside the disc else 0, 1 inside the disc else 0} (u8 x 4) of the dword whose byte 0 is pixel (dy, dx0) of the disc
struct DiscDwordWeight {
  uint32_t moment, count;
};
constexpr DiscDwordWeight disc_dword_weight(int dy, int dx0) {
  constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
  DiscDwordWeight w{0u, 0u};
  if (dy < -OR_R || dy > OR_R) return w;
  const int um = umax[dy < 0 ? -dy : dy];
  for (int b = 0; b < 4; ++b) {
    const int dx = dx0 + b;
    if (dx >= -um && dx <= um) {
      w.moment |= (uint32_t)(dx + OR_R) << (8 * b);
      w.count |= 1u << (8 * b);
    }
  }
  return w;
}
template <int ALIGN>
constexpr DiscWeightTable<ALIGN> make_disc_weight_table() {
  DiscWeightTable<ALIGN> r{};
  for (int e = 0; e < ALIGN * OR_WT; ++e) {
    const int sh = e / OR_WT, t = e - sh * OR_WT;
    if (t >= OR_NV) continue;
    const int row = t / (OR_DW / 2), c = t - row * (OR_DW / 2);
    for (int d = 0; d < 2; ++d) {
      const DiscDwordWeight w = disc_dword_weight(row - OR_R, 4 * (2 * c + d) - sh - OR_R);
      r.v[4 * e + d] = w.moment;
      r.v[4 * e + 2 + d] = w.count;
    }
  }
  return r;
}
__device__ __attribute__((aligned(128))) const DiscWeightTable<4> g_disc_weight_table = make_disc_weight_table<4>();

// The tiled form's disc weights, per dword: entry (a, j) = {moment, count} (disc_dword_weight), 8 bytes, for a patch whose
// first column sits a bytes into its first dword.  Rows r and 30 - r of the disc weigh alike, so the table holds the 16 rows
// dy = -15 .. 0 (OR_WFOLD); a row takes OR_WROW = 13 entries, its 12 dwords (three 16-byte pieces) and a pad, behind 3
// entries in front of row 0.  A patch that starts sh = 4 s + a bytes before its first column (sh < 16) weighs dword d of its
// piece (r, c) with entry (a, disc_weight_entry(r, c) + d + 3 - s): a lane reads the four of a piece as 32 contiguous bytes.
// Entries that fall into the previous row are its pad and its dwords 10 and 11, dx >= 22 there: 0, as the dwords left of the
// window are.
// The stride of 13 entries, 104 bytes, is for the LDS banks: the lanes of a wave-load hold neighbouring rows (disc_piece),
// and the 16 lanes that one half of a ds_read2_b64 serves together then read 16 x 8 bytes that start 26 dwords apart -- 16
// different even banks of the 32, no two lanes on one bank but where a group spans two piece columns.  With the rows end
// to end (12 entries, 96 bytes = 24 dwords) four lanes of every group met on each bank pair, and these reads alone kept the
// LDS array busy for 94 of the kernel's 210 cycles per keypoint (profiles/orient_lds_r10.md).  Folded, the table is 6,880
// bytes instead of 12,896: half the copy per workgroup, and room in LDS for the descriptor patch's wider rows.
constexpr int OR_WTD = 3 + OR_WROW * OR_WFOLD + 4;   // 215 entries per byte alignment, a whole number of uint4 in all
struct DiscWeightDwTable {
  uint32_t v[4 * OR_WTD * 2];
};
constexpr DiscWeightDwTable make_disc_weight_dw_table() {
  DiscWeightDwTable r{};
  for (int e = 0; e < 4 * OR_WTD; ++e) {
    const int a = e / OR_WTD, d = e - a * OR_WTD - 3;
    if (d < 0 || d >= OR_WROW * OR_WFOLD) continue;
    const int row = d / OR_WROW, col = d - row * OR_WROW;
    if (col >= 4 * OR_PC) continue;   // the pad
    const DiscDwordWeight w = disc_dword_weight(row - OR_R, 4 * col - a - OR_R);
    r.v[2 * e] = w.moment;
    r.v[2 * e + 1] = w.count;
  }
  return r;
}
__device__ __attribute__((aligned(128))) const DiscWeightDwTable g_disc_weight_dw_table = make_disc_weight_dw_table();
constexpr bool disc_weight_dw_table_matches() {   // every dword of every piece at all 16 alignments weighs as the definition says
  constexpr DiscWeightDwTable dw = make_disc_weight_dw_table();
  for (int sh = 0; sh < 16; ++sh)
    for (int r = 0; r < OR_ROWS; ++r)
      for (int c = 0; c < OR_PC; ++c)
        for (int d = 0; d < 4; ++d) {
          const int e = (sh & 3) * OR_WTD + disc_weight_entry(r, c) + d + 3 - (sh >> 2);
          if (e < 0 || e >= 4 * OR_WTD) return false;
          const DiscDwordWeight w = disc_dword_weight(r - OR_R, 16 * c + 4 * d - sh - OR_R);
          if (dw.v[2 * e] != w.moment || dw.v[2 * e + 1] != w.count) return false;
        }
  return true;
}
static_assert(disc_weight_dw_table_matches(), "DiscWeightDwTable must weigh every dword as disc_dword_weight");

// What orient_rbrief_kernel takes from the plane layout.  Row-major planes: patch rows start on the dword boundary below
// x - radius (4 alignments; EXACT: at x - radius itself).  Block-tiled planes: on the 16-byte boundary below it (16
// alignments) and are read as whole 16-byte block rows: three per row of the centroid patch (31 + 15 <= 48 bytes), three
// per row of the descriptor patch and one dword more where its 37 + a bytes pass 48 (TiledBriefRegs); its rows take 80
// bytes in LDS.
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
  static constexpr int ALIGN = 16, BR_DW = BR_DW_TILED;
  static constexpr int WT_VEC4 = 4 * OR_WTD * 2 / 4;   // uint4 entries of s_w (DiscWeightDwTable)
  // 7 waves per SIMD: <= 72 VGPRs (phase A keeps the centroid patches of ONE pair of keypoints in flight, 12 data registers;
  // the bin directions are loaded after phase A's patches, 8 registers fewer while they are in flight) and <= 23,405 B of
  // LDS (the weights per dword; ONE descriptor patch buffer per wave -- the ballots of keypoint k have consumed its patch
  // bytes before the patch of k + 1 is stored).  tests/test_orient_resources.py holds these figures.  The kernel uses
  // 18,720 B: 6,880 of weights (4 alignments x 215 entries: 16 folded rows of 13) and 4 x 37 x 80 of patch buffers; it was
  // bound by the LDS array's cycles, not by this budget, and both layouts are chosen for the banks (DiscWeightDwTable,
  // TiledBriefRegs).  18,720 B and the 63 registers the compiler then takes would admit 8 waves; VUS_OR_WPE_TILED_MAX says no.
  static constexpr int GRP = 1, BLUR_BUF = 1;   // GRP counts loader objects: one TiledDiscPair
  static constexpr bool BINS_AFTER_PHASE_A = true;
  typedef TiledDiscPair Disc;
  typedef TiledBriefRegs Brief;
  static constexpr const uint32_t* WEIGHT_TABLE = g_disc_weight_dw_table.v;   // s_w is a copy of it
  static constexpr const uint32_t* ROT_TABLE = g_rot_off_table_tiled.v;
  // Per-lane partial moments (sum dx I, sum dy I) of the two keypoints of a loaded pair, whose patches start sha / shb bytes
  // before their first columns.  The {moment, count} of a piece's four dwords are 32 contiguous bytes of s_w.  A piece that
  // was not read holds 0 and adds nothing, whatever weights it meets.
  static __device__ __forceinline__ void pair_moments(const uint4* s_w, const TiledDiscPair& pr, int sha, int shb, int lane, int& pa_a,
                                                      int& pq_a, int& pa_b, int& pq_b) {
    const bool second = lane >= TiledDiscPair::SPLIT;
    const int ea = (sha & 3) * OR_WTD + 3 - (sha >> 2), eb = (shb & 3) * OR_WTD + 3 - (shb >> 2);
    int mx[3], my[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      // the weights are laid out by the piece's row and column (disc_weight_entry), whatever slot the piece was dealt to
      const int e = (u == 0 ? ea : u == 2 ? eb : second ? eb : ea) + pr.weight_entry(u);
      const uint2* wd = reinterpret_cast<const uint2*>(s_w) + e;
      const uint32_t d[4] = {pr.v[u].x, pr.v[u].y, pr.v[u].z, pr.v[u].w};
      uint32_t sx = 0, rs = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint2 w = wd[j];
        sx = __builtin_amdgcn_udot4(d[j], w.x, sx, false);
        rs = __builtin_amdgcn_udot4(d[j], w.y, rs, false);
      }
      mx[u] = (int)sx - OR_R * (int)rs;
      my[u] = (pr.row(u) - OR_R) * (int)rs;
    }
    pa_a = mx[0] + (second ? 0 : mx[1]);
    pq_a = my[0] + (second ? 0 : my[1]);
    pa_b = mx[2] + (second ? mx[1] : 0);
    pq_b = my[2] + (second ? my[1] : 0);
  }
};
static_assert(2 * OR_R + 1 + 15 <= 16 * OR_PC && 2 * BR_R + 1 + 11 <= 48 && 2 * BR_R + 1 + 15 <= 52 && 52 <= 4 * BR_DW_TILED,
              "tiled patch rows: 16-byte aligned starts; descriptor rows of 48 bytes for a <= 11, 52 beyond");
static_assert(BR_DW_TILED % 4 == 0 && (BR_ROWS - 1) * 4 * BR_DW_TILED + 52 < (1 << 15),
              "descriptor patch in LDS: rows of whole uint4, every byte offset an int16 of g_rot_off_table_tiled");
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
//     GRP keypoints in flight; TILED: 3 dwordx4 per lane and PAIR of keypoints, one pair in flight) and are multiplied right
//     there with the disc weights (v_dot4_u32_u8; the weights of a lane's two dwords are ONE LDS read, those of a tiled
//     piece's four dwords two): no LDS round trip for the patch.  Per-lane partial moments of the eight keypoints
//     -> reduce-scatter (fold32 .. allsum8 above) -> lane 8g + j holds m10 / m01 of keypoint g and ranks bins 4j .. 4j+3.
//  B. descriptors, keypoint by keypoint: the 37-row patch of the smoothed image goes through LDS (BLUR_BUF buffers; the
//     next keypoint's rows and its bin's test offsets are in flight meanwhile), 8 byte reads + 4 compares per lane; the
//     ballots are written into lanes 4k + w of one register pair, so the eight descriptors leave in ONE 256-byte store.
// Its predecessor, one keypoint at a time: 232 vector instructions per keypoint (2.67 ms per 1000 stereo frames).
// ORDERED: slot s of an image is served with keypoint order[s] (vus_orient_order: the image's keypoints grouped by 64 x 64
// cell, the unused slots mapped to themselves), so that the eight keypoints of a wave and the 32 of a workgroup are
// neighbours and their patch rows share lines in flight; the outputs go to the keypoint's own index.  A schedule only.
// TILED: img and blur are block-tiled planes (include/vus_tiled.h, pitch = W).  OrGeom carries every difference: the
// patch loaders (which lane holds which 16-byte piece: disc_piece, brief_piece -- neighbouring lanes, neighbouring rows of
// one 128-byte line), the weight and test-offset tables, the patches in flight.  Phase B's LDS patch stays row-major
// (80-byte rows), so the ballots are those of the plain form.
template <bool EXACT, bool ORDERED, bool TILED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TILED ? VUS_OR_WPE_TILED : VUS_OR_WPE, TILED ? VUS_OR_WPE_TILED_MAX : 8))) void orient_rbrief_kernel(
    const uint8_t* __restrict__ img, const uint8_t* __restrict__ blur, int H, int W, int pitch,
    const uint32_t* __restrict__ kp_keys, const int* __restrict__ kp_count, int max_kp, const int* __restrict__ order,
    uint64_t* __restrict__ desc_out, uint8_t* __restrict__ angle_out, int n_img, int chunks_per_img) {
  typedef OrGeom<TILED, EXACT> G;
  __shared__ uint4 s_w[G::WT_VEC4];   // the disc weights for every byte alignment of a centroid patch (G::disc_weights)
  __shared__ __attribute__((aligned(TILED ? 16 : 8))) uint32_t s_blur[4][G::BLUR_BUF][BR_ROWS * G::BR_DW];
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
  int mom_dy[3];   // row-major planes: dy of the lane's three vectors (tiled: inside TiledDiscPair's pk)
  if constexpr (!TILED) {
#pragma unroll
    for (int u = 0; u < 3; ++u) mom_dy[u] = min(lane + 64 * u, OR_NV - 1) / (OR_DW / 2) - OR_R;
  }
  __syncthreads();   // the weight table is complete (the only workgroup-level synchronisation of the kernel)
  if (n_live == 0) {   // wave-uniform: nothing but defined contents for the unused slots
    if (lane < 4 * OR_KP_PER_WAVE && base_i + (lane >> 2) < max_kp) desc_out[((size_t)n * max_kp + base_i) * 4 + lane] = 0;
    if (lane < OR_KP_PER_WAVE && base_i + lane < max_kp) angle_out[(size_t)n * max_kp + base_i + lane] = 0;
    return;
  }

  // ---- phase A: centroid moments of the eight keypoints, GRP at a time
  int pa[8], pq[8];   // per-lane partials of m10 and m01
  if constexpr (TILED) {   // pairs of keypoints: three wave-loads hold both patches
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ya = __builtin_amdgcn_readlane(my_y, 2 * g), xa = __builtin_amdgcn_readlane(my_x, 2 * g);
      const int yb = __builtin_amdgcn_readlane(my_y, 2 * g + 1), xb = __builtin_amdgcn_readlane(my_x, 2 * g + 1);
      pa[2 * g] = pq[2 * g] = pa[2 * g + 1] = pq[2 * g + 1] = 0;
      if (2 * g < n_live) pr[0].load(im, H, W, ya, xa, yb, xb, 2 * g + 1 < n_live, lane);
      if (2 * g < n_live)
        G::pair_moments(s_w, pr[0], (xa - OR_R) & 15, (xb - OR_R) & 15, lane, pa[2 * g], pq[2 * g], pa[2 * g + 1], pq[2 * g + 1]);
    }
    // the first descriptor patch: behind the last moments, not behind the last centroid loads -- its up to 12 data registers
    // on top of the pair's 12 do not fit the 72; the reduce-scatter and the bin ranking run while it is in flight
    pb.load(bl, H, W, W, __builtin_amdgcn_readlane(my_y, 0), __builtin_amdgcn_readlane(my_x, 0), lane);
  } else {
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
    if constexpr (TILED) pb.store(patch, lane, __builtin_amdgcn_readlane(my_x, k));
    else pb.store(patch, lane);
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
