/* vus_retrieval.h -- loop-closure candidates by appearance: for every ordered pair of keyframes, how many of one
 * keyframe's strongest descriptors have a near neighbour among the other's (part of the C ABI of include/vus.h, which
 * includes this file; it can also be included on its own).
 *
 * Where it sits: in front of vus_hamming_match + vus_stereo_pair_pose (vus_loop.h).  Those measure a pair; this entry
 * point says which pairs are worth measuring, from the descriptors alone -- no pose enters, so a revisit is proposed
 * however far the odometry has drifted.  No vocabulary: the score is an exact all-pairs count.
 *
 *   desc      uint64 [n_img, max_kp, 4]   256-bit descriptors as vus_orient_rbrief writes them
 *   kp_count  int [n_img]                 valid slots per image
 *   q_img     int [n_q]   DEVICE: image number of query row q (the left image of keyframe f is image 2f)
 *   t_img     int [n_t]   DEVICE: image number of train column t
 *   t_limit   int [n_q]   DEVICE, or NULL: row q is computed for columns t < t_limit[q] only
 *   top, max_dist         descriptors used per image, Hamming bound of a near neighbour
 *   S         int32 [n_q, n_t]
 *
 * SEMANTICS.  For an image number m:  n(m) = min(max(kp_count[m], 0), max_kp, top)  if 0 <= m < n_img, else 0 (nothing is
 * indexed with such an m).  With nq = n(q_img[q]), nt = n(t_img[t]) and lim(q) = n_t if t_limit is NULL, else t_limit[q]
 * clamped to [0, n_t]:
 *
 *   S[q,t] = #{ i < nq :  min over j < nt of Hamming(desc[q_img[q], i], desc[t_img[t], j])  <=  max_dist }    for t < lim(q)
 *   S[q,t] = 0                                                                                                 for t >= lim(q)
 *
 * The minimum over an empty set is +infinity: S[q,t] = 0 when nt == 0 (and when nq == 0).  Every slot of S is written,
 * whatever it held.  Slots at or past nq / nt are never candidates, whatever they hold.  The score is directed: S[q,t]
 * counts descriptors of q, so S[q,t] != S[t,q] in general; S[q,q'] = nq when both rows name the same image (max_dist >= 0).
 * An image may appear in any number of rows and columns.  All sums are integer: the result does not depend on any order,
 * and two runs give equal bits.
 *
 * WHICH DESCRIPTORS.  The first `top` slots of an image.  Under vus_select_topk the slots are in ascending key order, that
 * is strongest first: the first `top` are the `top` strongest keypoints.  Under vus_select_grid the slots are cell-major
 * (cell by cell), so a prefix is a part of the image, not its best corners: use
 * top = max_kp there.
 *
 * Status -1 (VUS_E_INVALID) with vus_last_error() text that names the argument, before any launch, for: a null pointer
 * (t_limit may be NULL); n_img, n_q or n_t below 1; n_q * n_t above 2^31 - 1; max_kp outside 1..65535; top outside
 * 1..max_kp; max_dist outside 0..256.
 *
 * KERNEL (csrc/retrieve.hip).  The all-pairs Hamming distances are the FP4 block-scaled GEMM of the track matcher
 * (csrc/fp4_hamming.h: +-1 is exact in E2M1, dot = 256 - 2 Hamming, every accumulator an integer of magnitude <= 256,
 * exact in f32).  A workgroup of 256 threads holds 512 query descriptors of row q as B fragments in registers and walks
 * VUS_RETRIEVAL_TRAIN_BLOCK consecutive train columns, each expanded chunk by chunk (128 rows) into LDS as the A operand,
 * the next chunk's words loaded while this one's tiles run.  Per column of the tile the maximum dot over all rows of the
 * train image is kept; a query is a hit when it reaches 256 - 2 max_dist; a ballot and a popcount per column tile give one
 * integer add per wave and (q, t) into S, which the entry point zeroes on the stream first.  Workgroups whose train block
 * lies at or past lim(q) exit before they load anything.  One path only: there is no VALU form.
 *
 * NOT IN THIS ENTRY POINT: a symmetric or mutual score, a ratio test, tf-idf weighting, a vocabulary. */
#ifndef VUS_RETRIEVAL_H
#define VUS_RETRIEVAL_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_RETRIEVAL_MAX_KP 65535
#define VUS_RETRIEVAL_TRAIN_BLOCK 8

int vus_keyframe_similarity(const uint64_t* desc,      /* [n_img, max_kp, 4], as vus_orient_rbrief writes it */
                            const int* kp_count,       /* [n_img] */
                            int n_img, int max_kp,
                            const int* q_img, int n_q, /* DEVICE: image number of query row q (a keyframe's left image is 2f) */
                            const int* t_img, int n_t, /* DEVICE: image number of train column t */
                            const int* t_limit,        /* DEVICE [n_q] or NULL: row q is computed for t < t_limit[q] only */
                            int top, int max_dist,
                            int32_t* S,                /* [n_q, n_t] */
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_RETRIEVAL_H */
