// wn_cew.h -- launcher of the weighted cross-entropy head: class weights, label smoothing, position weights (wn_cew.hip).
// Tensors are channel-major (B, Q, T) fp32 like everywhere in the library; targets are int64.
#pragma once
#include "wn_device.h"

// Per loss position i = (b, t), t_start <= t < min(t_end[b], T), with s the logit column, y = target mod Q, p = softmax(s),
// w the (Q,) class weights (NULL: ones), r the (B, T) position weights (NULL: ones), W = sum_q w_q:
//   ce_i = -log p_y
//   l_i  = (1 - eps) w_y ce_i + (eps / Q) sum_q w_q (-log p_q)      (a class with w_q == 0 adds exactly 0; eps == 0: no sum)
//   g_iq = (1 - eps) w_y (p_q - [q == y]) + (eps / Q) (W p_q - w_q)
//   D = sum_i r_i w_{y_i} (normalize == 0, "weights") or n_loss (normalize == 1, "positions")
//   loss3[0] = loss_scale sum_i r_i l_i / D (0 with D == 0), loss3[1] = loss_scale sum_i ce_i / n_loss, loss3[2] = D
//   dlogits_iq = grad_scale r_i g_iq / D; exactly 0.0f off the loss positions, where r_i == 0 and with D == 0
//   pos_loss (nullable, (B, T)) = r_i l_i, 0 off the loss positions and where r_i == 0
// amax_out[0] = max |dlogits| (0 without dlogits).  Plain launches on st, no atomics, no host synchronisation: with weights of
// either kind under "weights" k_ce_divisor and its one-workgroup tail leave D and 1 / D in scratch (double); then the loss
// kernel leaves per-block partials of sum r l, sum ce and max |dlogits| as [3][sequence][column block], and k_cew_reduce adds
// them in double in a fixed order.  scratch: wn_cew_scratch_floats(B, T) floats, 8-byte aligned; every word read is written
// first.  Q <= 256: a workgroup of 4 waves holds all classes of 64 positions in registers and reads the logits once; wider
// heads take a plain one-thread-per-position loop.
long wn_cew_scratch_floats(int B, int T);
int wn_softmax_cew(const float* logits, const int64_t* target, const float* class_weights /*nullable*/,
                   const float* pos_weights /*nullable*/, float* dlogits /*nullable*/, float* pos_loss /*nullable*/, float* scratch,
                   int B, int T, int Q, int t_start, const int* t_end /*nullable*/, double n_loss, float eps, int normalize,
                   float grad_scale, float loss_scale, float* loss3, float* amax_out, wn_stream_t st);
