// Multiscale bootstrap weights drawn on the device, and the KH, SH and AU tests on the RELL
// matrices (gfx950 / CDNA4, wave64).
//
// The sampler.  Replicate rho = first_replicate + b draws n sites out of N = sum_p w[p]:
//   Philox4x32-10, key = seed, counter = (j, 0x72656C6C, rho lo, rho hi), j = 0 .. ceil(n/2) - 1
//   draw 2j   : x = c0 2^32 + c1          draw 2j+1 : x = c2 2^32 + c3   (unused when n is odd)
//   site = (x N) >> 64                    pattern: cum[p] <= site < cum[p+1]
// and W[b][p] counts the draws that landed in p.  Everything is integer arithmetic, so how the draws
// are dealt to lanes, waves and workgroups cannot change a bit.  A workgroup of four waves takes
// replicate after replicate; thread i takes the Philox calls i, i + 256, ...; every draw is a binary
// search in the prefix sum and one int32 atomic add into the replicate's histogram.  Up to
// kBootLdsPatterns patterns the histogram and the prefix sum are in LDS ((2 P + 1) words); beyond,
// or with MI_PHYLO_BOOT_HIST=global, the histogram is the workgroup's own row of the workspace and
// the prefix sum is read from memory.  The counts leave as doubles, a row's consecutive patterns by
// consecutive lanes.  No float atomics.
//
// The tests state the order of every floating-point sum; the file is compiled with
// -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_philox_device.h"

namespace miphylo {

namespace {

using dev::set_status;

constexpr uint32_t kBootStream = 0x72656C6Cu;  // the second counter word: apart from the samplers that use 0 and 1

// a pattern weight is a site count: a non-negative integer (NaN fails the first comparison); one of
// 2^31 or more counts as 2^31, which alone puts the total out of range
__device__ __forceinline__ bool boot_weight_ok(double w) { return w >= 0.0 && w <= 1.79769313486231570e308 && w == floor(w); }
__device__ __forceinline__ unsigned long long boot_weight_count(double w) {
  return boot_weight_ok(w) ? (unsigned long long)fmin(w, 2147483648.0) : 0ull;
}

// ---- the prefix sum, with the checks of the weights: one workgroup, once per call ----
// Thread i owns the patterns [i chunk, (i + 1) chunk); the 256 partial sums are scanned by thread 0.
__global__ __launch_bounds__(kBootThreads) void boot_prefix_kernel(BootArgs a) {
  __shared__ unsigned long long part[kBootThreads];
  __shared__ int refused;
  const int tid = threadIdx.x, P = a.P;
  const int chunk = (P + kBootThreads - 1) / kBootThreads;
  const int lo = min(tid * chunk, P), hi = min(lo + chunk, P);
  if (tid == 0) refused = 0;
  __syncthreads();
  unsigned long long sum = 0;
  for (int p = lo; p < hi; p++) {
    const double w = a.weights[p];
    if (!boot_weight_ok(w)) {
      set_status(a.status, kBootBadWeight, p);
      refused = 1;
    }
    sum += boot_weight_count(w);
  }
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    unsigned long long run = 0;
    for (int i = 0; i < kBootThreads; i++) {
      const unsigned long long x = part[i];
      part[i] = run;
      run += x;
    }
    bool ok = !refused;
    if (ok && !(run >= 1 && run < 2147483648ull)) {
      set_status(a.status, kBootBadTotal, 0);
      ok = false;
    }
    if (ok && a.expect_total >= 0 && run != (unsigned long long)a.expect_total) {
      set_status(a.status, kBootSitesNotTotal, 0);
      ok = false;
    }
    a.total[0] = ok ? (uint32_t)run : 0u;
    a.cum[P] = (uint32_t)run;
  }
  __syncthreads();
  unsigned long long run = part[tid];
  for (int p = lo; p < hi; p++) {
    const double w = a.weights[p];
    a.cum[p] = (uint32_t)run;
    run += boot_weight_count(w);
  }
}

// the pattern of a site: the p in [0, P) with cum[p] <= site < cum[p + 1] (site < cum[P])
__device__ __forceinline__ int boot_pattern(const uint32_t* cum, int P, uint32_t site) {
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid + 1] > site) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// GLOBAL: the histogram is row blockIdx.x of a.hist.  Its words are written by atomics, which are
// done in L2: they are zeroed and read back through L2 as well (relaxed agent-scope accesses), so
// that no line of this CU's L1 stands in for them.
template <bool GLOBAL>
__global__ __launch_bounds__(kBootThreads) void boot_sample_kernel(BootArgs a) {
  extern __shared__ uint32_t boot_lds[];  // !GLOBAL: histogram [P] | cum [P + 1]
  const int tid = threadIdx.x, P = a.P;
  const uint32_t N = a.total[0];
  int32_t* hist = GLOBAL ? a.hist + (size_t)blockIdx.x * P : reinterpret_cast<int32_t*>(boot_lds);
  const uint32_t* cum = a.cum;
  if (!GLOBAL) {
    uint32_t* c = boot_lds + P;
    for (int p = tid; p <= P; p += kBootThreads) c[p] = a.cum[p];
    cum = c;
  }
  const uint64_t n = a.sites, calls = (n + 1) >> 1;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    for (int p = tid; p < P; p += kBootThreads) {
      if (GLOBAL) __hip_atomic_store(hist + p, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else hist[p] = 0;
    }
    __syncthreads();  // (and the copy of cum, the first time round)
    const uint64_t rho = a.first_replicate + (uint64_t)b;
    if (N != 0) {
      for (uint64_t j = tid; j < calls; j += kBootThreads) {
        uint32_t c[4] = {(uint32_t)j, kBootStream, (uint32_t)rho, (uint32_t)(rho >> 32)};
        dev::philox4x32_10(c, a.seed);
        const uint64_t x0 = ((uint64_t)c[0] << 32) | c[1], x1 = ((uint64_t)c[2] << 32) | c[3];
        atomicAdd(hist + boot_pattern(cum, P, (uint32_t)__umul64hi(x0, (uint64_t)N)), 1);
        if (2 * j + 1 < n) atomicAdd(hist + boot_pattern(cum, P, (uint32_t)__umul64hi(x1, (uint64_t)N)), 1);
      }
    }
    __syncthreads();
    double* row = a.out + (size_t)b * P;
    for (int p = tid; p < P; p += kBootThreads) {
      const int32_t k = GLOBAL ? __hip_atomic_load(hist + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : hist[p];
      row[p] = (double)(uint32_t)k;
    }
    __syncthreads();  // the histogram is zeroed again only after every count has been read
  }
}

// zeroes of a call's integer counters (a kernel, so that a captured call holds kernel nodes only)
__global__ __launch_bounds__(256) void boot_zero_kernel(int32_t* words, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) words[i] = 0;
}

// ---- the tests ----
// t1 = argmax L, t2 = argmax over the others; the lowest index among equals (one wave: lane l takes
// trees l, l + 64, ... in ascending order, then rell_rows_kernel's butterfly)
__device__ __forceinline__ int topo_argmax(const double* L, int T, int skip, int lane) {
  constexpr int kNone = 0x7fffffff;
  double m = -__builtin_inf();
  int best = kNone;
  for (int t = lane; t < T; t += 64) {
    if (t == skip) continue;
    const double v = L[t];
    if (best == kNone || v > m) {
      m = v;
      best = t;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double om = __shfl_xor(m, off, 64);
    const int ob = __shfl_xor(best, off, 64);
    const bool take = ob != kNone && (best == kNone || om > m || (om == m && ob < best));
    m = take ? om : m;
    best = take ? ob : best;
  }
  return best == kNone ? -1 : best;
}
__global__ __launch_bounds__(64) void topo_select_kernel(TopoArgs a) {
  const int lane = threadIdx.x;
  const int t1 = topo_argmax(a.L, a.T, -1, lane);
  const int t2 = topo_argmax(a.L, a.T, t1, lane);
  if (lane == 0) {
    a.sel[0] = t1;
    a.sel[1] = t2;
  }
}

// mean[t] = (sum_b C[b][t]) / B: a lane per tree, one accumulator, b ascending
__global__ __launch_bounds__(64) void topo_means_kernel(TopoArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= a.T) return;
  const double* __restrict__ c = a.c + t;
  double sum = 0.0;
#pragma unroll 8
  for (int b = 0; b < a.B; b++) sum = sum + c[(size_t)b * a.T];
  a.mean[t] = sum / (double)a.B;
}

// zmax[b] = max_t Z[b][t], Z[b][t] = C[b][t] - mean[t]: a wave per replicate (a maximum has no order)
__global__ __launch_bounds__(256) void topo_row_max_kernel(TopoArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const double* __restrict__ row = a.c + (size_t)b * a.T;
  double m = -__builtin_inf();
  for (int t = lane; t < a.T; t += 64) {
    const double z = row[t] - a.mean[t];
    m = z > m ? z : m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double om = __shfl_xor(m, off, 64);
    m = om > m ? om : m;
  }
  if (lane == 0) a.zmax[b] = m;
}

// The SH and KH counts: a lane per tree and 64 replicates per workgroup, counted in registers, then
// one integer atomic add per (tree, workgroup).
//   SH: zmax[b] - Z[b][t] >= L[t1] - L[t]
//   KH: Z[b][ref] - Z[b][t] >= L[ref] - L[t],  ref = t1 for t != t1, t2 for t1; T = 1: every replicate
constexpr int kTopoCountRows = 64;
__global__ __launch_bounds__(64) void topo_count_kernel(TopoArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x, T = a.T;
  if (t >= T) return;
  const int t1 = a.sel[0], t2 = a.sel[1];
  const int ref = t == t1 ? t2 : t1;
  const double d_sh = a.L[t1] - a.L[t];
  const double d_kh = ref >= 0 ? a.L[ref] - a.L[t] : 0.0;
  const double mean_t = a.mean[t], mean_ref = ref >= 0 ? a.mean[ref] : 0.0;
  const int b0 = blockIdx.y * kTopoCountRows, b1 = min(b0 + kTopoCountRows, a.B);
  int sh = 0, kh = 0;
  for (int b = b0; b < b1; b++) {
    const double* __restrict__ row = a.c + (size_t)b * T;
    const double z = row[t] - mean_t;
    const double gap = a.zmax[b] - z;
    sh += gap >= d_sh ? 1 : 0;
    if (ref < 0) {
      kh += 1;
    } else {
      const double zr = row[ref] - mean_ref;
      const double diff = zr - z;
      kh += diff >= d_kh ? 1 : 0;
    }
  }
  atomicAdd(a.sh + t, sh);  // integer
  atomicAdd(a.kh + t, kh);
}

// The table, a lane per tree.  AU: weighted least squares of z_k on (sqrt r_k, 1 / sqrt r_k) over the
// usable scales in block order, five sums with one accumulator each.
__global__ __launch_bounds__(64) void topo_table_kernel(TopoArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x, T = a.T;
  if (t >= T) return;
  const double B = (double)a.B, N = (double)a.total[0];
  const double nan = __builtin_nan("");
  const double inv_sqrt_2pi = 0.3989422804014326779399461;
  double s11 = 0.0, s12 = 0.0, s22 = 0.0, t1 = 0.0, t2 = 0.0;
  int usable = 0;
  for (int k = 0; k < a.K; k++) {
    const int cnt = a.counts[(size_t)k * T + t], Bk = a.replicates[k];
    if (!(cnt > 0 && cnt < Bk)) continue;
    const double r = (double)a.sites[k] / N, x1 = sqrt(r), x2 = 1.0 / x1;
    const double pi = (double)cnt / (double)Bk, z = -normcdfinv(pi);
    const double phi = exp(-0.5 * (z * z)) * inv_sqrt_2pi;
    const double om = (double)Bk * (phi * phi) / (pi * (1.0 - pi));
    s11 = s11 + om * (x1 * x1);
    s12 = s12 + om * (x1 * x2);
    s22 = s22 + om * (x2 * x2);
    t1 = t1 + om * (x1 * z);
    t2 = t2 + om * (x2 * z);
    usable++;
  }
  double d = nan, c = nan, rss = nan, p_au = a.bp[t];
  if (usable >= 2) {
    const double det = s11 * s22 - s12 * s12;
    d = (t1 * s22 - t2 * s12) / det;
    c = (s11 * t2 - s12 * t1) / det;
    p_au = normcdf(c - d);
    rss = 0.0;
    for (int k = 0; k < a.K; k++) {
      const int cnt = a.counts[(size_t)k * T + t], Bk = a.replicates[k];
      if (!(cnt > 0 && cnt < Bk)) continue;
      const double r = (double)a.sites[k] / N, x1 = sqrt(r), x2 = 1.0 / x1;
      const double pi = (double)cnt / (double)Bk, z = -normcdfinv(pi);
      const double phi = exp(-0.5 * (z * z)) * inv_sqrt_2pi;
      const double om = (double)Bk * (phi * phi) / (pi * (1.0 - pi));
      const double e = z - d * x1 - c * x2;
      rss = rss + om * (e * e);
    }
  }
  double* row = a.table + (size_t)t * kTopoColumns;
  const double Lt = a.L[t];
  row[0] = Lt;
  row[1] = a.L[a.sel[0]] - Lt;
  row[2] = a.bp[t];
  row[3] = a.elw[t];
  row[4] = (double)a.kh[t] / B;
  row[5] = (double)a.sh[t] / B;
  row[6] = p_au;
  row[7] = d;
  row[8] = c;
  row[9] = rss;
  row[10] = (double)usable;
}

}  // namespace

void launch_boot_zero(int32_t* words, size_t count, hipStream_t s) {
  hipLaunchKernelGGL(boot_zero_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, words, count);
}

void launch_boot_prefix(const BootArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(boot_prefix_kernel, dim3(1), dim3(kBootThreads), 0, s, a);
}

void launch_boot_sample(const BootArgs& a, hipStream_t s) {
  if (a.global_hist) {
    const int grid = a.B < kBootGlobalRows ? a.B : kBootGlobalRows;
    hipLaunchKernelGGL(boot_sample_kernel<true>, dim3(grid), dim3(kBootThreads), 0, s, a);
  } else {
    const int grid = a.B < kBootLdsGrid ? a.B : kBootLdsGrid;
    const size_t lds = sizeof(uint32_t) * (2 * (size_t)a.P + 1);
    hipLaunchKernelGGL(boot_sample_kernel<false>, dim3(grid), dim3(kBootThreads), lds, s, a);
  }
}

void launch_topo_block0(const TopoArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(topo_select_kernel, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(topo_means_kernel, dim3((a.T + 63) / 64), dim3(64), 0, s, a);
  hipLaunchKernelGGL(topo_row_max_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(topo_count_kernel, dim3((a.T + 63) / 64, (a.B + kTopoCountRows - 1) / kTopoCountRows), dim3(64), 0,
                     s, a);
}

void launch_topo_table(const TopoArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(topo_table_kernel, dim3((a.T + 63) / 64), dim3(64), 0, s, a);
}

}  // namespace miphylo
