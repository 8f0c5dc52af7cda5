// The optimiser of a variational fit and the step's trace row (gfx950 / CDNA4,
// wave64).  The rule, the order of every operation and the trace row are in include/mi_phylo.h.
//   vi_check_kernel    a thread per element of the two tables: is its gradient finite, and is a
//                      split variable's sigma still finite and positive after the update; a flag
//                      per workgroup
//   vi_apply_kernel    every workgroup reads all the flags; unless one is set, Adam's moments and
//                      the ascent step, element by element
//   vi_finish_kernel   one wave: the flags once more, the K terms of the ELBO and the bound (64
//                      side by side, added lane after lane), the trace row, the state's scalars
// FP64 throughout, no atomics, plain vector stores, and the file is compiled without contraction
// (FLAGS_kernels_vi_fit): every operation is rounded once, every sum has one order.
#include <hip/hip_runtime.h>

#include "../../include/mi_phylo.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {

struct Element {
  const double* g;
  double *param, *m, *v;
  double step;
  bool sigma;
};

// element i of [0, P + 2V): the SBN parameters, then (mu, sigma) of every variable
__device__ __forceinline__ Element element_of(const ViUpdateArgs& a, size_t i) {
  Element e;
  if (i < (size_t)a.P) {
    e.g = a.g_sbn + i;
    e.param = a.phi + i;
    e.m = a.m_sbn + i;
    e.v = a.v_sbn + i;
    e.step = a.state->sbn_step;
    e.sigma = false;
  } else {
    const size_t j = i - (size_t)a.P;
    e.g = a.g_q + j;
    e.param = a.q_params + j;
    e.m = a.m_q + j;
    e.v = a.v_q + j;
    e.step = a.state->step[j & 1];
    e.sigma = (j & 1) != 0 && j < 2 * (size_t)a.S;
  }
  return e;
}

// m = (beta0 m) + ((1 - beta0) g), v = (beta1 v) + ((1 - beta1) (g g)),
// delta = (step (m / (1 - b0))) / (root + epsilon), root = sqrt(v / (1 - b1)); b0, b1 already
// advanced.  Where |g| > 2^500 the square g g may leave the range of a double (v is then +inf, and
// stored so), and the root is taken of the same sum in a scaled range: c = 2^-600,
// v' = (beta1 ((v c) c)) + ((1 - beta1) ((g c) (g c))), root = sqrt(v' / (1 - b1)) / c.  The
// products with c are exact but for the underflow of (v c) c, a term then 2^800 times smaller than
// the other: the root is the plain one wherever the plain one is finite.
constexpr double kHugeGradient = 0x1p500, kGradientScale = 0x1p-600;
__device__ __forceinline__ double adam(const ViUpdateArgs& a, const Element& e, double b0, double b1, double& m,
                                       double& v) {
  const double g = *e.g;
  m = (a.beta0 * *e.m) + ((1.0 - a.beta0) * g);
  v = (a.beta1 * *e.v) + ((1.0 - a.beta1) * (g * g));
  double root;
  if (fabs(g) > kHugeGradient) {
    const double gs = g * kGradientScale;
    const double vs = (a.beta1 * ((*e.v * kGradientScale) * kGradientScale)) + ((1.0 - a.beta1) * (gs * gs));
    root = sqrt(vs / (1.0 - b1)) / kGradientScale;
  } else {
    root = sqrt(v / (1.0 - b1));
  }
  return (e.step * (m / (1.0 - b0))) / (root + a.epsilon);
}

__device__ __forceinline__ bool finite(double x) { return x - x == 0.0; }

__global__ __launch_bounds__(256) void vi_check_kernel(ViUpdateArgs a) {
  const size_t N = (size_t)a.P + 2 * (size_t)a.V, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < N) {
    const Element e = element_of(a, i);
    if (!finite(*e.g)) {
      bad = true;
    } else if (e.sigma) {
      double m, v;
      const double sigma = *e.param + adam(a, e, a.state->b0 * a.beta0, a.state->b1 * a.beta1, m, v);
      bad = !(sigma > 0.0 && finite(sigma));
    }
  }
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) a.block_flags[blockIdx.x] = any ? 1 : 0;
}

__global__ __launch_bounds__(256) void vi_apply_kernel(ViUpdateArgs a, int blocks) {
  int bad = 0;
  for (int b = threadIdx.x; b < blocks; b += 256) bad |= a.block_flags[b];
  if (__syncthreads_or(bad)) return;  // a failed step changes neither table nor moment
  const size_t N = (size_t)a.P + 2 * (size_t)a.V, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const Element e = element_of(a, i);
  double m, v;
  const double delta = adam(a, e, a.state->b0 * a.beta0, a.state->b1 * a.beta1, m, v);
  *e.m = m;
  *e.v = v;
  *e.param = *e.param + delta;
}

// term k of the objective at beta = 1
__device__ __forceinline__ double term_of(const ViUpdateArgs& a, int k) {
  return ((a.log_lik[k] + a.log_prior[k]) - a.log_q_top[k]) - a.log_q_branch[k];
}

__global__ __launch_bounds__(64) void vi_finish_kernel(ViUpdateArgs a, int blocks) {
  const int lane = threadIdx.x;
  int bad = 0;
  for (int b = lane; b < blocks; b += 64) bad |= a.block_flags[b];
  const bool failed = __ballot(bad != 0) != 0ull;
  // the maximum of the K terms (a NaN is never the maximum: it reaches the sums instead)
  double top = -INFINITY;
  for (int k = lane; k < a.K; k += 64) {
    const double f = term_of(a, k);
    if (f > top) top = f;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double other = __shfl_xor(top, off, 64);
    if (other > top) top = other;
  }
  double sum = 0.0, sum_exp = 0.0;
  for (int k0 = 0; k0 < a.K; k0 += 64) {
    const int k = k0 + lane;
    const double f = k < a.K ? term_of(a, k) : 0.0;
    const double x = k < a.K ? exp(f - top) : 0.0;
    const int count = min(a.K - k0, 64);
    for (int j = 0; j < count; j++) {
      sum = sum + __shfl(f, j, 64);
      sum_exp = sum_exp + __shfl(x, j, 64);
    }
  }
  if (lane != 0) return;
  ViState* s = a.state;
  const int64_t t = s->t;
  double step0 = s->step[0], step1 = s->step[1];
  if (failed) {
    step0 = step0 / 2.0;
    step1 = step1 / 2.0;
  } else {
    step0 = step0 * a.decay;
    step1 = step1 * a.decay;
    s->b0 = s->b0 * a.beta0;
    s->b1 = s->b1 * a.beta1;
    s->a = s->a + 1;
  }
  s->step[0] = step0;
  s->step[1] = step1;
  const double row[6] = {vi_beta(t, s->anneal_steps),
                         sum / (double)a.K,
                         top == -INFINITY ? top : (top + log(sum_exp)) - log((double)a.K),
                         step0,
                         step1,
                         failed ? 0.0 : 1.0};
  for (int j = 0; j < 6; j++) {
    if (a.trace && t < a.max_steps) a.trace[6 * (size_t)t + j] = row[j];
    if (a.out_row) a.out_row[j] = row[j];
  }
  s->t = t + 1;
}

}  // namespace

int vi_update_blocks(int P, int V) { return (int)(((size_t)P + 2 * (size_t)V + 255) / 256); }

void launch_vi_update(const ViUpdateArgs& a, hipStream_t s) {
  const int blocks = vi_update_blocks(a.P, a.V);
  hipLaunchKernelGGL(vi_check_kernel, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(vi_apply_kernel, dim3(blocks), dim3(256), 0, s, a, blocks);
  hipLaunchKernelGGL(vi_finish_kernel, dim3(1), dim3(64), 0, s, a, blocks);
}

}  // namespace miphylo
