// Fit control: the host half of the reference's epoch loop (scripts_experiments/train_GNN.py:73-111) as one launch of one
// workgroup behind every epoch's three graphs -- ReduceLROnPlateau on the validation loss, the early-stopping counters, the
// copy of the best weights and the loss log all stay in device memory, so a fit is enqueued ahead of the GPU and the host
// reads one flag per control interval (hcatgnet_amd/fit.py; the contract is in include/hcatgnet_hip.h: hcg_fit_control_args).
// The arithmetic is float64 and never contracted: each product, quotient and comparison is the one Python makes, which is
// what keeps a device fit bitwise the host loop (fit.FitControl restates this state machine and is its CPU oracle).
#include "common.h"

namespace {

constexpr int FIT_THREADS = 1024;

__global__ __launch_bounds__(FIT_THREADS) void k_fit_control(hcg_fit_control_args a, int64_t nvec) {
#pragma clang fp contract(off)
  __shared__ int s_snapshot;
  hcg_fit_state s;
  bool live = false;
  if (threadIdx.x == 0) {
    s = *a.state;
    int snapshot = 0;
    live = !s.stopped && s.epoch >= 0 && s.epoch < a.max_epochs;
    if (live) {
      const double train = *a.sums[0] / a.denom[0], val = *a.sums[1] / a.denom[1], test = *a.sums[2] / a.denom[2];
      if (s.epoch % a.control_every == 0) {
        // torch.optim.lr_scheduler.ReduceLROnPlateau.step(val), mode "min", threshold_mode "rel"
        s.last_epoch += 1;
        if (val < s.sched_best * a.rel_epsilon) {
          s.sched_best = val;
          s.num_bad_epochs = 0;
        } else {
          s.num_bad_epochs += 1;
        }
        if (s.cooldown_counter > 0) {
          s.cooldown_counter -= 1;
          s.num_bad_epochs = 0;
        }
        if (s.num_bad_epochs > a.patience) {
          const double scaled = s.lr * a.factor;
          const double lr_new = a.min_lr > scaled ? a.min_lr : scaled;      // Python's max(scaled, min_lr)
          if (s.lr - lr_new > a.eps) {
            s.lr = lr_new;
            *a.lr_dev = (float)lr_new;
          }
          s.cooldown_counter = a.cooldown;
          s.num_bad_epochs = 0;
        }
        // the loop's own bookkeeping
        if (val < s.val_best) {
          s.val_best = val;
          s.best_epoch = s.epoch;
          s.stall = 0;
          snapshot = 1;
        } else {
          s.stall += 1;
        }
        s.stopped = s.stall > a.early_stopping ? 1 : 0;
      }
      double* row = a.log + 4 * (int64_t)s.epoch;
      row[0] = train;
      row[1] = val;
      row[2] = test;
      row[3] = s.lr;
      s.epoch += 1;
      s.epochs_counted += 1;
    }
    s_snapshot = snapshot;
  }
  __syncthreads();
  if (s_snapshot) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(a.param);
    float4* __restrict__ dst = reinterpret_cast<float4*>(a.best);
    for (int64_t i = threadIdx.x; i < nvec; i += FIT_THREADS) dst[i] = src[i];
    for (int64_t i = 4 * nvec + threadIdx.x; i < a.n; i += FIT_THREADS) a.best[i] = a.param[i];
  }
  __syncthreads();
  if (live) *a.state = s;                               // (thread 0 alone is ever live) the state goes last
}

}  // namespace

// reached through hcg_update_dev (optim.hip): `fit_control` of its argument struct
int hcg_fit_control_launch(const hcg_fit_control_args* a, hipStream_t stream) {
  if (!a || !a->sums[0] || !a->sums[1] || !a->sums[2] || !a->state || !a->lr_dev || !a->param || !a->best || !a->log)
    return HCG_ERR_INVALID_ARG;
  for (int k = 0; k < 3; ++k)
    if (!(a->denom[k] > 0.0)) return HCG_ERR_INVALID_ARG;
  if (a->n <= 0 || a->max_epochs < 1 || a->control_every < 1 || a->patience < 0 || a->cooldown < 0 || a->early_stopping < 0)
    return HCG_ERR_INVALID_ARG;
  if (!(a->factor < 1.0) || a->rel_epsilon != a->rel_epsilon || a->min_lr != a->min_lr || a->eps != a->eps)
    return HCG_ERR_INVALID_ARG;
  if (a->param == a->best || ((uintptr_t)a->param | (uintptr_t)a->best) % sizeof(float) || (uintptr_t)a->state % sizeof(double) ||
      (uintptr_t)a->log % sizeof(double))
    return HCG_ERR_INVALID_ARG;
  const bool aligned = (((uintptr_t)a->param | (uintptr_t)a->best) % sizeof(float4)) == 0;
  const int64_t nvec = aligned ? a->n / 4 : 0;
  hipLaunchKernelGGL(k_fit_control, dim3(1), dim3(FIT_THREADS), 0, stream, *a, nvec);
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}
