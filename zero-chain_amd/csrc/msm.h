// Pippenger multi-scalar multiplication over BLS12-381 G1 / G2 for gfx950.
//
// Replaces bellman 0.1.0's multiexp (multiexp.rs; restated in SURVEY.md A.2) behind the 8
// call sites inside create_proof (reference entry: core/proofs/src/confidential.rs:149).
// bellman: window c = ceil(ln n), one CPU task per window, 2^c - 1 buckets per window, running
// sum per window, c doublings per window fold.  The group element computed is the same; the
// schedule is rebuilt for a GPU with 288 GB of HBM:
//
//   * bases are fixed (the CRS), so EVERY doubling 2^k * P_i, k = 0..254, is precomputed once
//     into a [255][n] affine table (2.7 GB for the Transfer key, 25.7 GB for 2^20 bases).  No
//     doubling is ever done at proving time, all digits of a scalar share ONE set of buckets,
//     and bucket reduction runs once per job.
//   * with a multiple available at every bit position the scalar is recoded in width-c NAF:
//     odd signed digits |d| < 2^(c-1) at arbitrary positions, on average one non-zero digit
//     per c + 1 bits (bellman: one per c bits) over only 2^(c-2) buckets (bellman: 2^c - 1).
//   * the same memory buys a larger digit set: the tables bound to a circuit also hold m * 2^k * P_i for the odd m = 3, 5, ...
//     (slice 255 j + k for m = 2 j + 1: 3.7 -> 29.9 GB for the Transfer key with eight), a digit m * b (b odd, b < 2^(c-1))
//     goes into bucket b through the slice of m, and a scalar has a digit per c + 1 + g bits, g = 0.6 / 1.25 / 1.85 for two /
//     four / eight multiples (msm_types.h MsmRecode, msm_recode.h msm_wnaf_mult) - buckets, reduction and tail exactly as they were.
//   * (digit, point) pairs are counting-sorted by bucket (histogram with returned ranks ->
//     per-job exclusive scan -> scatter).  A bucket is cut into tasks of <= seg points and
//     the tasks of the whole launch are ordered by length, so the 64 lanes of a wave walk
//     equally long runs of XYZZ mixed additions (8M+2S, dev_curve.h) with no idle lanes.
//   * buckets are reduced with chunked running sums: chunk t of length L yields
//     sum_k (2(tL+k)+1) B_{tL+k}; chunk results are summed on rows of 16 lanes (coop_tail.cpp).
//
// A "job" is one MSM instance (one query of one proof).  Jobs of a batch that live in the
// same group share every launch; `MsmJob` carries the per-job pointers.
//
// The kernels by pass, a header each:
//   msm_types.h          MsmJob, MsmSelSet, MsmOcc, MsmRecode, the MSM_* sizes: all that host code outside the group sees
//   msm_recode.h         the recodings of a scalar into digits: msm_wnaf, msm_wnaf_mult, msm_vb_digit, msm_digits
//   msm_sort.h           passes 1-4: the counting sort of the pairs (LDS / two-level) and the task order (msm_g1.cpp only)
//   msm_accumulate.h     pass 5: the compiled accumulation, its second pass, the calibration inputs
//   msm_asm_g1.h         the generated G1 loops' wrappers: accumulation and level 1 of the reduction (msm_g1.cpp only)
//   msm_asm_g2.h         the generated G2 loop's wrappers in both forms (msm_g2.cpp only)
//   msm_reduce.h         passes 5b, 5c, 6: the merge of task partials and level 1 of the bucket reduction on lanes
//   msm_inverse.h        field inversions and to_affine (device functions)
//   msm_points.h         curve_b, fld_import / fld_export, the decoders of the encodings (device functions)
//   msm_point_kernels.h  import, decode, check, table build, export and normalisation kernels
// This header includes all of them for the stand-alone benchmarks (tools/ubench); the product's units include what they launch.
#pragma once
#include "msm_types.h"
#include "msm_recode.h"
#include "msm_sort.h"
#include "msm_accumulate.h"
#include "msm_asm_g1.h"
#include "msm_asm_g2.h"
#include "msm_reduce.h"
#include "msm_inverse.h"
#include "msm_points.h"
#include "msm_point_kernels.h"
