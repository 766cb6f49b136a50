/*
 * rfuse_optim.h -- the optimiser ABI of librfuse_hip.so: one Adam step (torch/optim/adam.py:_single_tensor_adam with amsgrad=False, maximize=False,
 * capturable=False) over a LIST of tensors in as few launches as the list allows, the last torch-only stage of both trainers' step
 * (trainer/train_retrieval.py:37, trainer/train_refinement.py:185-203).
 *
 * A ninth header, in the vocabulary and with the conventions of the other eight (extern "C", no allocation, stream-ordered on `stream`, 0 or an
 * RF_E_* code from every `int` function whose last parameter is `stream`, rf_last_error() for the message, no `double` scalar, argument checks
 * before any device is touched).  The other headers stay as they are.
 *
 * rf_adam_step reads a HOST table of `count` records of rf_adam_step_record_bytes() = 72 bytes each, little endian, no padding between members:
 *
 *     offset  0  uint64   param        device pointers to `n` contiguous float32 each; any 4-byte alignment (a view at an odd element offset is
 *     offset  8  uint64   grad         fine: a record whose four pointers are not all 16-byte aligned is updated with 4-byte accesses)
 *     offset 16  uint64   exp_avg
 *     offset 24  uint64   exp_avg_sq
 *     offset 32  int64    n            1 <= n < 2^31
 *     offset 40  float32  neg_step     -step_size,  step_size = lr / (1 - beta1^t)
 *     offset 44  float32  bc2_sqrt     sqrt(1 - beta2^t)
 *     offset 48  float32  w1           1 - beta1
 *     offset 52  float32  beta2
 *     offset 56  float32  w2           1 - beta2
 *     offset 60  float32  eps
 *     offset 64  float32  weight_decay
 *     offset 68  4 bytes, not read
 *
 * The scalars are per record because t, lr and weight_decay differ per tensor and per parameter group; the caller computes them in float64 where
 * torch computes them and rounds once to float32.  Per element, the float32 roundings of torch's CPU kernels in torch's order: every operation
 * correctly rounded by itself, except the three multiply-adds that those kernels fuse (one rounding each), written fma() here:
 *
 *     g  = fma(weight_decay, param, grad)                    only when weight_decay != 0          grad.add(param, alpha = weight_decay)
 *     m  = |w1| < 0.5 ? fma(w1, g - m, m) : fma(-(g - m), 1 - w1, g)                                m.lerp_(g, w1)
 *     v  = fma(w2 * g, g, v * beta2)                                                               v.mul_(beta2).addcmul_(g, g, value = w2)
 *     p  = p + (neg_step * m) / (sqrt(v) / bc2_sqrt + eps)                                         p.addcdiv_(m, denom, value = neg_step)
 *
 * m, v and p are written back, grad is only read.  No reductions and no atomics: the same inputs give the same bits on every call; NaN and
 * +-inf propagate as the expressions above propagate them.  The table is copied into the kernel arguments at launch (nothing is read from it
 * after the call returns, nothing is cached between calls, no device memory is allocated, the host is not synchronised): at most
 * rf_adam_step_max_tensors() records per launch, ceil(count / rf_adam_step_max_tensors()) launches per call.  A workgroup updates one segment of
 * rf_adam_step_segment() consecutive elements of one tensor.  The tensors of one call must not overlap.
 */
#ifndef RFUSE_OPTIM_H
#define RFUSE_OPTIM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* records one launch takes (>= 32), bytes of one record of the host table (72), elements one workgroup updates */
int rf_adam_step_max_tensors(void);
int rf_adam_step_record_bytes(void);
int rf_adam_step_segment(void);

/* records: HOST pointer to `count` >= 1 records as above.  RF_E_INVALID: a null or misaligned (not 4-byte) pointer, n < 1; RF_E_UNSUPPORTED: n >= 2^31.
 * Every record is checked before the first launch. */
int rf_adam_step(const void* records, int count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
