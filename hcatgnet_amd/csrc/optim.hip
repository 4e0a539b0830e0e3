// Adam step for the model's parameters in ONE launch per contiguous segment (the step right
// after the path).  The reference uses torch.optim.Adam(lr, eps=1e-9) (model/networks.py:38) on 8 small
// tensors (16 641 floats): through torch's foreach implementation that is ~10 multi-tensor launches and
// ~0.5 ms of host time per step -- more than the whole fwd+bwd here.  Same update rule as torch
// (amsgrad=False, weight_decay=0, maximize=False):
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2
//   p -= (lr / (1 - b1^t)) * m / ( sqrt(v) / sqrt(1 - b2^t) + eps )
// The capturable form also runs the reference's other two optimisers with torch's defaults (HCG_UPDATE_SGD, _RMSPROP).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                              float bc1, float bc2_sqrt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float mi = m[i], vi = v[i];
  p[i] = hcg_adam_update(p[i], g[i], mi, vi, b1, b2, eps, lr / bc1, bc2_sqrt);
  m[i] = mi;
  v[i] = vi;
}

}  // namespace

// step = 1-based step count of this update; bias corrections are computed on the host in double like torch
extern "C" int hcg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                             float beta1, float beta2, float eps, int64_t step, hcg_stream_t stream) {
  if (n < 0 || step < 1 || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq))) return HCG_ERR_INVALID_ARG;
  if (n == 0) return HCG_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)hcg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, n, lr, beta1, beta2, eps, (float)bc1, (float)sqrt(bc2));
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}

namespace {

// step count and learning rate read from device memory (hipGraph-capturable), one kernel per update rule (HCG_UPDATE_*).
// Adam's bias corrections in double like torch's host computation.  The last workgroup to take a ticket (step_dev[2], zero
// between launches) publishes step + 1 and re-zeroes the ticket; step_dev[1], the exchange stamp, is not touched (a plain
// update exchanges nothing).  RMSprop: v = square_avg, b2 = alpha; SGD reads no state.
// SSE: `g` = [n summed SSE/2-gradients | SSE | count] (data-parallel form HCG_LOSS_SSE): the
// gradient of sqrt(MSE) over all ranks' graphs is g * 1 / (count * sqrt(SSE / count)); written back in place.
template <int RULE, bool SSE>
__global__ __launch_bounds__(256) void k_update_dev(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, const float* __restrict__ lr_dev, float b1,
                                                    float b2, float eps, int* __restrict__ step_dev, float* __restrict__ loss) {
  const int t = step_dev[0] + 1;
  const float lr = lr_dev[0];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float gs = 1.0f;
  if (SSE) {
    const float sse = g[n], cnt = g[n + 1], mse = sse / cnt, lv = sqrtf(mse);
    gs = 1.0f / (cnt * lv);
    if (i == 0) { loss[0] = lv; loss[1] = mse; }
  }
  if (i < n) {
    float bc1 = 1.0f, bc2_sqrt = 1.0f;
    if (RULE == HCG_UPDATE_ADAM) {
      bc1 = (float)(1.0 - hcg_powi((double)b1, t));
      bc2_sqrt = (float)sqrt(1.0 - hcg_powi((double)b2, t));
    }
    const float gi = g[i] * gs;
    if (SSE) g[i] = gi;
    if (RULE == HCG_UPDATE_ADAM) {
      float mi = m[i], vi = v[i];
      p[i] = hcg_adam_update(p[i], gi, mi, vi, b1, b2, eps, lr / bc1, bc2_sqrt);
      m[i] = mi;
      v[i] = vi;
    } else if (RULE == HCG_UPDATE_RMSPROP) {
      float vi = v[i];
      p[i] = hcg_rmsprop_update(p[i], gi, vi, b2, eps, lr);
      v[i] = vi;
    } else {
      p[i] = hcg_sgd_update(p[i], gi, lr);
    }
  }
  __syncthreads();                                     // every thread of this block has read the step word
  if (threadIdx.x == 0) {
    const int ticket = __hip_atomic_fetch_add(&step_dev[2], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == (int)gridDim.x - 1) {
      __hip_atomic_store(&step_dev[2], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&step_dev[0], t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int RULE>
void launch_update_dev(float* p, float* g, float* m, float* v, int64_t n, const float* lr_dev, float b1, float b2, float eps,
                       int32_t* step_dev, float* loss, hipStream_t stream) {
  const dim3 grid((unsigned)hcg_cdiv(n, 256));
  if (loss) hipLaunchKernelGGL((k_update_dev<RULE, true>), grid, dim3(256), 0, stream, p, g, m, v, n, lr_dev, b1, b2, eps, (int*)step_dev, loss);
  else hipLaunchKernelGGL((k_update_dev<RULE, false>), grid, dim3(256), 0, stream, p, g, m, v, n, lr_dev, b1, b2, eps, (int*)step_dev, nullptr);
}

__global__ __launch_bounds__(256) void k_sse_finalize(float* __restrict__ g, int64_t n, float* __restrict__ loss) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float sse = g[n], cnt = g[n + 1], mse = sse / cnt, lv = sqrtf(mse);
  if (i == 0) { loss[0] = lv; loss[1] = mse; }
  if (i < n) g[i] *= 1.0f / (cnt * lv);
}

}  // namespace

extern "C" int hcg_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                 const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_dev,
                                 hcg_stream_t stream) {
  if (n <= 0 || !param || !grad || !exp_avg || !exp_avg_sq || !lr_dev || !step_dev) return HCG_ERR_INVALID_ARG;
  launch_update_dev<HCG_UPDATE_ADAM>(param, const_cast<float*>(grad), exp_avg, exp_avg_sq, n, lr_dev, beta1, beta2, eps,
                                     step_dev, nullptr, (hipStream_t)stream);
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}

extern "C" int hcg_adam_step_dev_sse(float* param, float* flat, float* exp_avg, float* exp_avg_sq, int64_t n,
                                     const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_dev, float* loss,
                                     hcg_stream_t stream) {
  if (n <= 0 || !param || !flat || !exp_avg || !exp_avg_sq || !lr_dev || !step_dev || !loss) return HCG_ERR_INVALID_ARG;
  launch_update_dev<HCG_UPDATE_ADAM>(param, flat, exp_avg, exp_avg_sq, n, lr_dev, beta1, beta2, eps, step_dev, loss,
                                     (hipStream_t)stream);
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}

extern "C" int hcg_update_dev(const hcg_update_args* a, hcg_stream_t stream_) {
  if (a && a->fit_control) return hcg_fit_control_launch(a->fit_control, (hipStream_t)stream_);      // (fit.hip)
  if (!a || a->n <= 0 || !a->grad) return HCG_ERR_INVALID_ARG;
  const hipStream_t stream = (hipStream_t)stream_;
  if (!a->param) {                                     // the SSE form's scale and loss alone
    if (!a->loss) return HCG_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_sse_finalize, dim3((unsigned)hcg_cdiv(a->n, 256)), dim3(256), 0, stream, a->grad, a->n, a->loss);
    HCG_CHECK_LAUNCH();
    return HCG_OK;
  }
  if (!a->lr_dev || !a->step_dev) return HCG_ERR_INVALID_ARG;
  switch (a->update_rule) {
    case HCG_UPDATE_ADAM:
      if (!a->exp_avg || !a->exp_avg_sq) return HCG_ERR_INVALID_ARG;
      launch_update_dev<HCG_UPDATE_ADAM>(a->param, a->grad, a->exp_avg, a->exp_avg_sq, a->n, a->lr_dev, a->beta1, a->beta2,
                                         a->eps, a->step_dev, a->loss, stream);
      break;
    case HCG_UPDATE_SGD:
      launch_update_dev<HCG_UPDATE_SGD>(a->param, a->grad, nullptr, nullptr, a->n, a->lr_dev, 0.f, 0.f, 0.f, a->step_dev,
                                        a->loss, stream);
      break;
    case HCG_UPDATE_RMSPROP:
      if (!a->exp_avg_sq) return HCG_ERR_INVALID_ARG;
      launch_update_dev<HCG_UPDATE_RMSPROP>(a->param, a->grad, nullptr, a->exp_avg_sq, a->n, a->lr_dev, 0.f, a->beta2, a->eps,
                                            a->step_dev, a->loss, stream);
      break;
    default:
      return HCG_ERR_INVALID_ARG;
  }
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}
