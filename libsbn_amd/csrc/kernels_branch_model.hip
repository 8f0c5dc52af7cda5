// PSP indexing and the log-normal branch-length models of a variational step (DESIGN.md 4.23;
// gfx950 / CDNA4, wave64).  The definitions (what a PSP is, the order of the draws, every sum's
// order, the order of evaluation of every term) are in include/mi_phylo.h.
//   psp_table_kernel       one workgroup: the flag of every PCSP, its exclusive scan (a ballot and a
//                          population count per wave, the four waves' totals through LDS), the gather
//   psp_index_kernel       a thread per entry of [T][R][2n-3]: the k = 0 slots through the table
//   branch_sample_kernel   a wave per tree: 64 edges side by side (parameters, the Philox normal,
//                          x, theta and the edge's log q term), the two sums lane after lane
//   branch_terms_kernel    a thread per (tree, edge): the two terms c0, c1; a thread per tree: log_f
//   branch_keys_kernel / radix sort / branch_runs_kernel
//                          the key, stable sort and run-head scheme of kernels_sbn_vi.hip with the
//                          two components of a run added side by side
// FP64 throughout, one integer atomic (the status word), and the file is compiled without
// contraction (FLAGS_kernels_branch_model): every sum has the one order the header states.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>  // before rocprim: its texture iterator calls memset from host code

#include <rocprim/rocprim.hpp>

#include "../../include/mi_phylo.h"
#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_philox_device.h"

namespace miphylo {

namespace {
using namespace dev;

// ---- PSP indexing ----
// PCSP i is a PSP when its sister is the complement of its focal clade.  out[i] = S + the number of
// PSPs before i, or -1.
__global__ __launch_bounds__(256) void psp_table_kernel(PspTableArgs a) {
  __shared__ int wave_total[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;  // PSPs before this round's 256 entries
  for (int i0 = 0; i0 < a.C; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    const bool flag = i < a.C && a.pcsp_clades[3 * (size_t)i] == (a.pcsp_clades[3 * (size_t)i + 1] ^ 1);
    const unsigned long long mask = __ballot(flag);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    int mine = base;
    for (int w = 0; w < wave; w++) mine += wave_total[w];
    if (i < a.C) a.out_psp_of_pcsp[i] = flag ? a.S + mine + before : -1;
    base += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.out_counts[0] = a.S;
    a.out_counts[1] = a.S + base;
  }
}

// entry q = (t R + r) E + v: row 0 the rootsplit of edge v, row 1 the PSP of slot (2v, 0), row 2
// that of slot (2v + 1, 0); whatever is not a variable is V
__global__ __launch_bounds__(256) void psp_index_kernel(PspIndexArgs a) {
  const int E = 2 * a.n - 3;
  const size_t Q = (size_t)a.T * a.R * E;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const size_t row = q / E, t = row / a.R;
  const int v = (int)(q - row * E), r = (int)(row - t * a.R);
  int out = a.V;
  if (r == 0) {
    const int j = a.root_index[t * E + v];
    if (j >= 0 && j < a.S) out = j;
  } else {
    const int d = 2 * v + (r == 2 ? 1 : 0);
    const int j = a.slot_index[(t * 2 * E + d) * 3];
    if (j >= a.S && j < a.S + a.C) {
      const int p = a.psp_of_pcsp[j - a.S];
      if (p >= a.S && p < a.V) out = p;
    }
  }
  a.out_index[q] = out;
}

// ---- the log-normal models ----
__device__ __forceinline__ void report(int32_t* status, int tree, int edge) {
  if (atomicCAS(status, 0, (int)kBranchModelBadParam) == 0) {
    status[1] = tree;
    status[3] = edge;
  }
}

// mu and sigma of edge v of tree t: the rows' parameters added in ascending r from 0; false (and
// the status word) unless sigma is finite and positive and mu is not NaN
__device__ __forceinline__ bool edge_params(const int32_t* index, const double* q_params, int V, int R, int E, size_t t,
                                            int v, int32_t* status, double& mu, double& sigma) {
  mu = 0.0;
  sigma = 0.0;
  for (int r = 0; r < R; r++) {
    const int j = index[(t * R + r) * E + v];
    if (j >= 0 && j < V) {
      mu = mu + q_params[2 * (size_t)j];
      sigma = sigma + q_params[2 * (size_t)j + 1];
    }
  }
  const bool good = sigma > 0.0 && sigma < INFINITY && mu == mu;
  if (!good) report(status, (int)t, v);
  return good;
}

// (the standard normal of edge v of sample s: philox_normal, mi_phylo_philox_device.h)
constexpr double kHalfLog2Pi = 0.91893853320467274178;  // log(2 pi) / 2

__global__ __launch_bounds__(256) void branch_sample_kernel(BranchSampleArgs a) {
  const int lane = threadIdx.x & 63, E = 2 * a.n - 3;
  const size_t t = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= (size_t)a.T) return;  // (the whole wave)
  const uint64_t s = (uint64_t)((a.vi ? vi_sample_base(*a.vi) : a.first_sample) + (int64_t)t);
  double sum_q = 0.0, sum_theta = 0.0;
  for (int v0 = 0; v0 < E; v0 += 64) {
    const int v = v0 + lane;
    double term = 0.0, theta = 0.0;
    if (v < E) {
      double mu, sigma;
      edge_params(a.index, a.q_params, a.V, a.R, E, t, v, a.status, mu, sigma);
      const double eps = a.epsilon_in ? a.epsilon_in[t * E + v] : philox_normal(a.seed, s, (uint32_t)v);
      const double x = mu + sigma * eps;
      theta = exp(x);
      term = ((x + log(sigma)) + kHalfLog2Pi) + 0.5 * (eps * eps);
      a.out_bl[t * (E + 1) + v] = theta;
      a.out_epsilon[t * E + v] = eps;
    }
    const int count = min(E - v0, 64);
    for (int j = 0; j < count; j++) {
      sum_q = sum_q + __shfl(term, j, 64);
      sum_theta = sum_theta + __shfl(theta, j, 64);
    }
  }
  if (lane == 0) {
    a.out_bl[t * (E + 1) + E] = 0.0;
    a.out_log_q[t] = -sum_q;
    a.out_log_prior[t] = (double)E * log(a.prior_rate) - a.prior_rate * sum_theta;
  }
}

// c0 = w (d theta + 1), c1 = w (((d theta) eps + eps) + 1 / sigma), d = g - rate; and log_f
__global__ __launch_bounds__(256) void branch_terms_kernel(BranchGradientArgs a) {
  const int E = 2 * a.n - 3;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)a.T) {
    const double beta = a.vi ? vi_beta(a.vi->t, a.vi->anneal_steps) : a.beta;
    a.out_log_f[i] = ((beta * a.log_likelihoods[i] + a.log_prior[i]) - (a.log_q_topology ? a.log_q_topology[i] : 0.0)) -
                     a.log_q_branch[i];
  }
  if (i >= (size_t)a.T * E) return;
  const size_t t = i / E;
  const int v = (int)(i - t * E);
  double mu, sigma;
  edge_params(a.index, a.q_params, a.V, a.R, E, t, v, a.status, mu, sigma);
  const double w = a.weights ? a.weights[t] : 1.0;
  const double d = a.branch_gradient[t * (E + 2) + v] - a.prior_rate;
  const double dt = d * a.bl[t * (E + 1) + v], eps = a.epsilon[i];
  a.terms[2 * i] = w * (dt + 1.0);
  a.terms[2 * i + 1] = w * ((dt * eps + eps) + 1.0 / sigma);
}

// entry q of [T][R][E]; entries without a variable get the key V and sort behind the rest
__global__ __launch_bounds__(256) void branch_keys_kernel(BranchGradientArgs a) {
  const size_t Q = (size_t)a.T * a.R * (2 * a.n - 3);
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q < 2 * (size_t)a.V) a.out_gradient[q] = 0.0;
  if (q >= Q) return;
  const int32_t j = a.index[q];
  a.keys[q] = j >= 0 && j < a.V ? (uint32_t)j : (uint32_t)a.V;
  a.vals[q] = (uint32_t)q;
}

// the terms of entry q are those of its (tree, edge)
__device__ __forceinline__ size_t term_of(const BranchGradientArgs& a, uint32_t q) {
  const uint32_t E = (uint32_t)(2 * a.n - 3), row = q / E;
  return (size_t)(row / (uint32_t)a.R) * E + (q - row * E);
}

// sorted position p: the head of a run adds the run in ascending entry number (the sort is stable),
// one accumulator per component.  A run of up to 16 entries is added by its head's lane; a longer
// one by the whole wave, 64 entries side by side, added lane after lane: the same additions in the
// same order.
constexpr int kShortRun = 16;
__global__ __launch_bounds__(256) void branch_runs_kernel(BranchGradientArgs a) {
  const size_t Q = (size_t)a.T * a.R * (2 * a.n - 3);
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t k = p < Q ? a.keys2[p] : (uint32_t)a.V;
  const bool head = k < (uint32_t)a.V && (p == 0 || a.keys2[p - 1] != k);
  bool is_long = false;
  if (head) {
    size_t end = p + 1;
    while (end < Q && end - p <= kShortRun && a.keys2[end] == k) end++;
    is_long = end - p > kShortRun;
    if (!is_long) {
      double s0 = 0.0, s1 = 0.0;
      for (size_t q = p; q < end; q++) {
        const size_t i = term_of(a, a.vals2[q]);
        s0 = s0 + a.terms[2 * i];
        s1 = s1 + a.terms[2 * i + 1];
      }
      a.out_gradient[2 * (size_t)k] = s0;
      a.out_gradient[2 * (size_t)k + 1] = s1;
    }
  }
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const size_t begin = p - lane + src;  // (the head's position, the same in every lane)
    const uint32_t key = (uint32_t)__shfl((int)k, src, 64);
    double s0 = 0.0, s1 = 0.0;
    for (size_t q0 = begin;; q0 += 64) {
      const size_t q = q0 + lane;
      const bool in = q < Q && a.keys2[q] == key;
      const size_t i = in ? term_of(a, a.vals2[q]) : 0;
      const double c0 = in ? a.terms[2 * i] : 0.0, c1 = in ? a.terms[2 * i + 1] : 0.0;
      const unsigned long long out = ~__ballot(in);
      const int count = out ? __ffsll((long long)out) - 1 : 64;
      for (int j = 0; j < count; j++) {
        s0 = s0 + __shfl(c0, j, 64);
        s1 = s1 + __shfl(c1, j, 64);
      }
      if (out) break;
    }
    if (lane == 0) {
      a.out_gradient[2 * (size_t)key] = s0;
      a.out_gradient[2 * (size_t)key + 1] = s1;
    }
  }
}

unsigned bits_for(size_t values) {  // keys are 0 .. values - 1
  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < values) bits++;
  return bits;
}

unsigned blocks_of(size_t threads) { return (unsigned)((std::max<size_t>(threads, 1) + 255) / 256); }

}  // namespace

void launch_psp_table(const PspTableArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(psp_table_kernel, dim3(1), dim3(256), 0, s, a);
}

void launch_psp_index(const PspIndexArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(psp_index_kernel, dim3(blocks_of((size_t)a.T * a.R * (2 * a.n - 3))), dim3(256), 0, s, a);
}

void launch_branch_sample(const BranchSampleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(branch_sample_kernel, dim3((unsigned)(((size_t)a.T + 3) / 4)), dim3(256), 0, s, a);
}

// (room for keys of any width: a reservation does not know V)
size_t branch_model_sort_tmp_bytes(size_t entries) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (uint32_t*)nullptr, entries, 0, 32, (hipStream_t)0);
  return bytes;
}

int launch_branch_gradient(const BranchGradientArgs& a, hipStream_t s) {
  const size_t E = 2 * (size_t)a.n - 3, Q = (size_t)a.T * a.R * E;
  hipLaunchKernelGGL(branch_terms_kernel, dim3(blocks_of((size_t)a.T * E)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(branch_keys_kernel, dim3(blocks_of(std::max<size_t>(Q, 2 * (size_t)a.V))), dim3(256), 0, s, a);
  size_t sort_bytes = a.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(a.sort_tmp, sort_bytes, a.keys, a.keys2, a.vals, a.vals2, Q, 0,
                                bits_for((size_t)a.V + 1), s) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(branch_runs_kernel, dim3(blocks_of(Q)), dim3(256), 0, s, a);
  return 0;
}

}  // namespace miphylo
