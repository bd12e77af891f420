// frontend_common.h -- what two or more units of the stereo ORB front-end for gfx950 (MI355X) share.  The front-end is
// FAST-9/16 + NMS + smoothing (detect.hip), top-K selection (select.hip), intensity-centroid orientation + rotated BRIEF
// (orient.hip), brute-force Hamming matching (match.hip), the track ids, the factor emitter and the get_landmarks
// triangulation of the reference, batch.py:144-176 (track.hip), the optional scale pyramid (pyramid.hip), and the keyframe
// similarity that proposes loop-closure candidates from the descriptors (retrieve.hip; it shares fp4_hamming.h with match.hip).
//
// Replaces the external `gtsam_vio/ImageProcessorNodelet` the reference wires in at
// launch/stereo.launch:33-55 (its output is what batch.py:149-154 consumes).  Algorithm
// definitions (integer, bit-exact) are stated in include/vus.h; the CPU oracle under oracle/
// restates them independently for the parity tests.
//
// Design notes (MI355X), every stage:
//  * everything is batched over images: grid.z / grid.y = image, so one launch covers the whole
//    resident stream and fills the 256 CUs.
//
// Internal linkage, like factor_common.h and device_util.h: every unit that includes it gets its own copy.  A helper
// with one user lives with its user.
#pragma once
#include "vus_common.h"
#include "../../include/vus_tiled.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// inclusive scan over the 64 lanes of a wave (DPP row shifts / broadcasts)
__device__ __forceinline__ int wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xe, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xc, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);
  return v;
}

int check_image_args(const void* img, int n_img, int H, int W, int pitch) {
  VUS_REQUIRE(img != nullptr, "image pointer is null");
  VUS_REQUIRE(n_img >= 0 && n_img <= (1 << 20), "n_img=%d out of range [0, 2^20]", n_img);
  VUS_REQUIRE(H >= 7 && W >= 7, "image %dx%d too small (need >= 7x7)", W, H);
  VUS_REQUIRE(pitch >= W, "pitch %d < W %d", pitch, W);
  VUS_REQUIRE((long long)H * W <= (1ll << VUS_KEY_POS_BITS), "H*W=%lld exceeds 2^24", (long long)H * W);
  return VUS_OK;
}

// the planes of include/vus_tiled.h: whole 16 x 8 blocks, 16-byte aligned (the raw copy's dwordx4 stores)
static int check_tiled_args(const void* a, const void* b, int H, int W) {
  VUS_REQUIRE(a != nullptr && b != nullptr, "tiled plane pointer is null");
  VUS_REQUIRE(W % VUS_TILE_BW == 0 && H % VUS_TILE_BH == 0, "tiled planes need W %% %d == 0 and H %% %d == 0 (got %dx%d)",
              VUS_TILE_BW, VUS_TILE_BH, W, H);
  VUS_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0, "tiled planes must be 16-byte aligned");
  return VUS_OK;
}

}  // namespace
