// The variational fit over the rooted trees of the subsplit DAG (gfx950 / CDNA4,
// wave64).  The rules (every sum's order, every term's order of evaluation) are in include/mi_phylo.h.
//   gp_vi_normalize_kernel      a lane per block: the maximum, the sum of exp(phi - m) in ascending entry
//                               order with one accumulator, then log q and q of every entry
//   gp_vi_branch_sample_kernel  a wave per tree: 64 nodes side by side (the entry's mu and sigma, the
//                               Philox normal, x, theta and the node's log q term), the two sums lane after
//                               lane (the scheme of branch_sample_kernel)
//   gp_vi_terms_kernel          a thread per (tree, node): c0, c1 with the likelihood gradient gathered
//                               through new_id; a thread per tree: log_f
//   gp_vi_keys_kernel / radix sort / gp_vi_runs_kernel
//                               ONE stable sort of (entry, position) serves both ordered sums: the head of
//                               an entry's run adds the run's terms and its trees' factors in ascending
//                               position, one accumulator each; a run of more than 16 positions is added
//                               by the whole wave, 64 side by side and lane after lane: the same additions
//                               in the same order
//   gp_vi_blocks_kernel         a lane per block: the block's sum of G in ascending entry order, then
//                               out[j] = G_j - q_j sum
// FP64 and integers only; the one atomic is the integer compare-and-swap of the status word; plain
// vector stores; nothing spins.  Compiled without contraction (FLAGS_kernels_gp_vi).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>  // before rocprim: its texture iterator calls memset from host code

#include <rocprim/rocprim.hpp>

#include "../../include/mi_phylo.h"
#include "mi_phylo_device.h"
#include "mi_phylo_device_utils.h"
#include "mi_phylo_gp_vi.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_philox_device.h"

namespace miphylo {

namespace {
using namespace dev;

// block B: 0 the rootsplits; 1 + 2 (v - n) + c: (node v, clade c)
__device__ __forceinline__ void block_of(const int32_t* block_range, int n, int R, int B, int& begin, int& end) {
  begin = 0, end = R;
  if (B > 0) {
    const size_t at = ((size_t)(n + (B - 1) / 2) * 2 + ((B - 1) & 1)) * 2;
    begin = block_range[at];
    end = block_range[at + 1];
  }
}

// ---- log-normalisation ----
// l_e = (phi_e - m) - log(sum_i exp(phi_i - m)), q_e = exp(l_e); a block that is all -inf: l = -inf, q = 0
__global__ __launch_bounds__(64) void gp_vi_normalize_kernel(GpViNormArgs a) {
  const int blocks = 1 + 2 * (a.nodes - a.n);
  const int B = blockIdx.x * 64 + threadIdx.x;
  if (B >= blocks) return;
  int begin, end;
  block_of(a.block_range, a.n, a.R, B, begin, end);
  double m = -INFINITY;
  for (int j = begin; j < end; j++) {
    const double x = a.log_params[j];
    if (x != x || x == INFINITY) set_status(a.status, kSbnBadParam, j);
    if (x > m) m = x;
  }
  double sum = 0.0;
  for (int j = begin; j < end; j++) sum = sum + (m == -INFINITY ? 0.0 : exp(a.log_params[j] - m));
  const double log_sum = log(sum);
  for (int j = begin; j < end; j++) {
    const double l = m == -INFINITY ? -INFINITY : (a.log_params[j] - m) - log_sum;
    if (a.out_log_q) a.out_log_q[j] = l;
    a.out_q[j] = exp(l);
  }
}

// ---- the branch lengths ----
__device__ __forceinline__ void report(int32_t* status, int code, int tree, int node) {
  if (atomicCAS(status, 0, code) == 0) {
    status[1] = tree;
    status[3] = node;
  }
}

// mu and sigma of node v of tree t: its entry's row; false (and the status word) at a sentinel, or unless
// sigma is finite and positive and mu is not NaN
__device__ __forceinline__ bool entry_params(const int32_t* entries, const double* q_params, int G, int N, size_t t, int v,
                                             int32_t* status, double& mu, double& sigma) {
  mu = 0.0;
  sigma = 0.0;
  const int e = entries[t * N + v];
  if (e < 0 || e >= G) {
    report(status, kGpViBadEntry, (int)t, v);
    return false;
  }
  mu = q_params[2 * (size_t)e];
  sigma = q_params[2 * (size_t)e + 1];
  const bool good = sigma > 0.0 && sigma < INFINITY && mu == mu;
  if (!good) report(status, kBranchModelBadParam, (int)t, v);
  return good;
}

constexpr double kHalfLog2Pi = 0.91893853320467274178;  // log(2 pi) / 2

__global__ __launch_bounds__(256) void gp_vi_branch_sample_kernel(GpViSampleArgs a) {
  const int lane = threadIdx.x & 63, N = 2 * a.n - 1, E = N - 1;
  const size_t t = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= (size_t)a.T) return;  // (the whole wave)
  const uint64_t s = (uint64_t)((a.vi ? vi_sample_base(*a.vi) : a.first_sample) + (int64_t)t);
  double sum_q = 0.0, sum_theta = 0.0;
  for (int v0 = 0; v0 < E; v0 += 64) {
    const int v = v0 + lane;
    double term = 0.0, theta = 0.0;
    if (v < E) {
      double mu, sigma;
      entry_params(a.entries, a.q_params, a.G, N, t, v, a.status, mu, sigma);
      const double eps = a.epsilon_in ? a.epsilon_in[t * E + v] : philox_normal(a.seed, s, (uint32_t)v);
      const double x = mu + sigma * eps;
      theta = exp(x);
      term = ((x + log(sigma)) + kHalfLog2Pi) + 0.5 * (eps * eps);
      a.out_lengths[t * N + v] = theta;
      a.out_epsilon[t * E + v] = eps;
    }
    const int count = min(E - v0, 64);
    for (int j = 0; j < count; j++) {
      sum_q = sum_q + __shfl(term, j, 64);
      sum_theta = sum_theta + __shfl(theta, j, 64);
    }
  }
  if (lane == 0) {
    a.out_lengths[t * N + E] = 0.0;
    a.out_log_q[t] = -sum_q;
    a.out_log_prior[t] = (double)E * log(a.prior_rate) - a.prior_rate * sum_theta;
  }
}

// c0 = w (d theta + 1), c1 = w (((d theta) eps + eps) + 1 / sigma), d = g[new_id] - rate; and log_f
__global__ __launch_bounds__(256) void gp_vi_terms_kernel(GpViTermsArgs a) {
  const int N = 2 * a.n - 1, E = N - 1;
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
  entry_params(a.entries, a.q_params, a.G, N, t, v, a.status, mu, sigma);
  const double w = a.weights ? a.weights[t] : 1.0;
  const int u = a.new_id[t * N + v];  // (an unrooted edge: below 2n-3; a refused tree has -1)
  const double g = u >= 0 && u < E - 1 ? a.branch_gradient[t * N + u] : NAN;
  const double d = g - a.prior_rate;
  const double dt = d * a.lengths[t * N + v], eps = a.epsilon[i];
  a.terms[2 * i] = w * (dt + 1.0);
  a.terms[2 * i + 1] = w * ((dt * eps + eps) + 1.0 / sigma);
}

// ---- the per-entry ordered sums ----
// position p = t N + v; a sentinel gets the key G and sorts behind the rest
__global__ __launch_bounds__(256) void gp_vi_keys_kernel(GpViSumsArgs a) {
  const size_t Q = (size_t)a.T * (2 * a.n - 1);
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (a.terms && p < 2 * (size_t)a.G) a.out_q_gradient[p] = 0.0;
  if (a.factors && p < (size_t)a.G) a.usage[p] = 0.0;
  if (p >= Q) return;
  const int32_t e = a.entries[p];
  a.keys[p] = e >= 0 && e < a.G ? (uint32_t)e : (uint32_t)a.G;
  a.vals[p] = (uint32_t)p;
}

// what position p adds to its entry: its node's two terms (the root's slot has none) and its tree's factor
struct Summand {
  double c0, c1, f;
};
__device__ __forceinline__ Summand summand_of(const GpViSumsArgs& a, uint32_t p) {
  const uint32_t N = (uint32_t)(2 * a.n - 1), t = p / N, v = p - t * N;
  Summand s{0.0, 0.0, 0.0};
  if (a.terms && v + 1 < N) {
    const size_t i = (size_t)t * (N - 1) + v;
    s.c0 = a.terms[2 * i];
    s.c1 = a.terms[2 * i + 1];
  }
  if (a.factors) s.f = a.factors[t];
  return s;
}

__device__ __forceinline__ void store_sums(const GpViSumsArgs& a, uint32_t k, double s0, double s1, double sf) {
  if (a.terms) {
    a.out_q_gradient[2 * (size_t)k] = s0;
    a.out_q_gradient[2 * (size_t)k + 1] = s1;
  }
  if (a.factors) a.usage[k] = sf;
}

constexpr int kShortRun = 16;
__global__ __launch_bounds__(256) void gp_vi_runs_kernel(GpViSumsArgs a) {
  const size_t Q = (size_t)a.T * (2 * a.n - 1);
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t k = p < Q ? a.keys2[p] : (uint32_t)a.G;
  const bool head = k < (uint32_t)a.G && (p == 0 || a.keys2[p - 1] != k);
  bool is_long = false;
  if (head) {
    size_t end = p + 1;
    while (end < Q && end - p <= kShortRun && a.keys2[end] == k) end++;
    is_long = end - p > kShortRun;
    if (!is_long) {
      double s0 = 0.0, s1 = 0.0, sf = 0.0;
      for (size_t q = p; q < end; q++) {
        const Summand x = summand_of(a, a.vals2[q]);
        s0 = s0 + x.c0;
        s1 = s1 + x.c1;
        sf = sf + x.f;
      }
      store_sums(a, k, s0, s1, sf);
    }
  }
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const size_t begin = p - lane + src;  // (the head's position, the same in every lane)
    const uint32_t key = (uint32_t)__shfl((int)k, src, 64);
    double s0 = 0.0, s1 = 0.0, sf = 0.0;
    for (size_t q0 = begin;; q0 += 64) {
      const size_t q = q0 + lane;
      const bool in = q < Q && a.keys2[q] == key;
      Summand x{0.0, 0.0, 0.0};
      if (in) x = summand_of(a, a.vals2[q]);
      const unsigned long long out = ~__ballot(in);
      const int count = out ? __ffsll((long long)out) - 1 : 64;
      for (int j = 0; j < count; j++) {
        s0 = s0 + __shfl(x.c0, j, 64);
        s1 = s1 + __shfl(x.c1, j, 64);
        sf = sf + __shfl(x.f, j, 64);
      }
      if (out) break;
    }
    if (lane == 0) store_sums(a, key, s0, s1, sf);
  }
}

// out[j] = G_j - q_j sum_{i in block(j)} G_i, the block's sum in ascending entry order
__global__ __launch_bounds__(64) void gp_vi_blocks_kernel(GpViSumsArgs a) {
  const int blocks = 1 + 2 * (a.nodes - a.n);
  const int B = blockIdx.x * 64 + threadIdx.x;
  if (B >= blocks) return;
  int begin, end;
  block_of(a.block_range, a.n, a.R, B, begin, end);
  double total = 0.0;
  for (int j = begin; j < end; j++) total = total + a.usage[j];
  for (int j = begin; j < end; j++) a.out_gradient[j] = a.usage[j] - a.q[j] * total;
}

unsigned bits_for(size_t values) {  // keys are 0 .. values - 1
  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < values) bits++;
  return bits;
}

unsigned blocks_of(size_t threads, unsigned per) { return (unsigned)((std::max<size_t>(threads, 1) + per - 1) / per); }

}  // namespace

void launch_gp_vi_normalize(const GpViNormArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gp_vi_normalize_kernel, dim3(blocks_of(1 + 2 * (size_t)(a.nodes - a.n), 64)), dim3(64), 0, s, a);
}

void launch_gp_vi_branch_sample(const GpViSampleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gp_vi_branch_sample_kernel, dim3(blocks_of((size_t)a.T, 4)), dim3(256), 0, s, a);
}

void launch_gp_vi_terms(const GpViTermsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gp_vi_terms_kernel, dim3(blocks_of((size_t)a.T * (2 * a.n - 2), 256)), dim3(256), 0, s, a);
}

int launch_gp_vi_sums(const GpViSumsArgs& a, hipStream_t s) {
  const size_t Q = (size_t)a.T * (2 * a.n - 1);
  hipLaunchKernelGGL(gp_vi_keys_kernel, dim3(blocks_of(std::max<size_t>(Q, 2 * (size_t)a.G), 256)), dim3(256), 0, s, a);
  size_t sort_bytes = a.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(a.sort_tmp, sort_bytes, a.keys, a.keys2, a.vals, a.vals2, Q, 0, bits_for((size_t)a.G + 1), s) !=
      hipSuccess)
    return 1;
  hipLaunchKernelGGL(gp_vi_runs_kernel, dim3(blocks_of(Q, 256)), dim3(256), 0, s, a);
  if (a.factors)
    hipLaunchKernelGGL(gp_vi_blocks_kernel, dim3(blocks_of(1 + 2 * (size_t)(a.nodes - a.n), 64)), dim3(64), 0, s, a);
  return 0;
}

}  // namespace miphylo
