/*
 * catfish_hip_ext.h -- entry points of libcatfish_hip.so next to the core C ABI of catfish_hip.h (same library, same
 * dialect, same conventions: 0 = ok, negative = failure, cf_last_error() has the message; every launch on `stream`, no host
 * synchronisation, no allocation, graph-capturable).
 *
 * Global-norm gradient clipping and a non-finite-step guard in front of the optimizer of the training step:
 *
 *     S   = sum over the n floats of grads of double(g_i)^2, in float64, in a fixed order
 *     g   = sqrt(S)
 *     s32 = float32(clip_norm / max(g, clip_norm))       (tf.clip_by_global_norm; 1.0f exactly for g <= clip_norm, and
 *                                                         1.0f without CF_CLIP_SCALE)
 *     the optimizer consumes float32(g_i * s32) in place of g_i
 *     with CF_CLIP_SKIP_NONFINITE the step is skipped when S is not finite (some g_i is NaN or +-Inf) or loss[0] is not
 *     finite: no variable, slot or packed weight changes and the step counter stays
 *
 * record: device double[4], updated on the stream by cf_clip_norm and read by cf_opt_step_guarded:
 *     [0] g of the last step   [1] the scale applied, s32; CF_CLIP_SKIPPED (-1) when the last step was skipped
 *     [2] steps clipped so far (s32 < 1)   [3] steps skipped so far
 * The caller zeroes it once; the host reads it whenever it likes.
 */
#ifndef CATFISH_HIP_EXT_H
#define CATFISH_HIP_EXT_H

#include <stdint.h>

#include "catfish_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a signature of this header changes; cf_ext_abi_version() returns the value the library was built with. */
#define CF_EXT_ABI_VERSION 1

#define CF_CLIP_SCALE 1              /* flags: scale the gradients to a global norm of at most clip_norm */
#define CF_CLIP_SKIP_NONFINITE 2     /* flags: skip a step whose gradients or loss are not finite        */
#define CF_CLIP_SKIPPED -1           /* record[1] after a skipped step                                   */
#define CF_CLIP_CHUNK 16384          /* floats per partial sum of the norm                               */

int cf_ext_abi_version(void);

/* Doubles of workspace cf_clip_norm needs for n gradient floats: one partial sum per chunk of CF_CLIP_CHUNK floats
 * (0 for n <= 0). */
int64_t cf_clip_workspace_doubles(int64_t n);

/* The global norm of grads[0 .. n) and the decision for this step, into record.  Two launches: one workgroup per chunk sums
 * its chunk's squares in float64 (every thread a fixed subset in ascending order, then a fixed tree); one workgroup folds the
 * partials (thread j those of chunks j, j + 256, ... in ascending order, then the same tree), takes the root and writes the
 * record.  No float atomics: equal inputs give equal bits.  flags: CF_CLIP_SCALE and / or CF_CLIP_SKIP_NONFINITE, at least
 * one; clip_norm: finite and > 0 with CF_CLIP_SCALE, ignored without.  loss: device float[1] of this step, or NULL (then
 * only the gradients decide a skip).  grads must be 16-byte aligned. */
int cf_clip_norm(cf_model* m, const float* grads, int64_t n, double clip_norm, int32_t flags, const float* loss, double* workspace,
                 int64_t workspace_doubles, double* record, void* stream);

/* cf_opt_step with the gradients scaled on the fly by record[1], and nothing at all on a skipped step (record[1] ==
 * CF_CLIP_SKIPPED): no update, no re-tiling, step_count stays.  With record[1] == 1 the result is bit-identical to
 * cf_opt_step's.  record: the one cf_clip_norm wrote earlier on the same stream. */
int cf_opt_step_guarded(cf_model* m, int32_t kind, float* params, const float* grads, float* slot1, float* slot2, int64_t n, float lr,
                        double* step_count, const int32_t* pack_idx, const float* pack_scale, float* packed, int64_t n_packed,
                        const double* record, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CATFISH_HIP_EXT_H */
