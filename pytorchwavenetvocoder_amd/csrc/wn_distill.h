// wn_distill.h -- launcher of the soft-target (knowledge distillation) loss head (wn_distill.hip).
// Tensors are channel-major (B, Q, T) fp32 like everywhere in the library; targets are int64.
#pragma once
#include "wn_device.h"

// Per live position (t_start <= t < t_end[b]), with s the student's and u the teacher's logit column and y = target mod Q:
//   ce = logsumexp(s) - s_y
//   kl = sum_q P_q (log P_q - log S_q),  P = softmax(u / tau), S = softmax(s / tau); a class with P_q == 0 adds exactly 0
//   l  = (1 - alpha) ce + alpha tau^2 kl
//   dlogits_q = gs * ((1 - alpha) (softmax(s)_q - [q == y]) + alpha tau (S_q - P_q));  exactly 0 on every other position
// alpha == 1: the target is not read (may be NULL), ce is 0 everywhere.  alpha == 0: l = ce (kl is still reported).
// loss3[0] = scale * sum l, loss3[1] = scale * sum ce, loss3[2] = scale * sum kl; pos_loss (nullable, (B, T)) = l, 0 off the live
// set; amax_out[0] = max |dlogits| (0 without dlogits).  Two plain launches on st: the loss kernel leaves per-block partial
// sums of ce and kl and partial maxima as [3][sequence][column block] in scratch (wn_distill_scratch_floats(B, T) floats, every
// word it reads is written first), the reduction adds them in double in a fixed order.  No atomics: same inputs, same bits.
// Q <= 256: a workgroup of 4 waves holds all classes of 64 positions in registers and reads both inputs once; wider heads take
// a plain one-thread-per-position loop.
long wn_distill_scratch_floats(int B, int T);
int wn_softmax_distill(const float* logits, const float* teacher, const int64_t* target /*nullable with alpha == 1*/,
                       float* dlogits /*nullable*/, float* pos_loss /*nullable*/, float* scratch, int B, int T, int Q, int t_start,
                       const int* t_end /*nullable*/, float alpha, float tau, float gs, float scale, float* loss3, float* amax_out,
                       wn_stream_t st);
