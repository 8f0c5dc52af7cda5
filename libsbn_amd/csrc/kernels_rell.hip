// RELL re-summation of per-pattern log-likelihoods, its reductions, and the tree-mixture
// marginal (gfx950 / CDNA4, wave64).
//
//   C[b][t] = sum_p W[b][p] s[t][p]      W: [B][P] replicate weights, s: [T][P] log L_p per tree
//
// The product runs on v_mfma_f64_16x16x4_f64.  Its operand maps (header of kernels_aa.hip): lane
// l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], and register r of the result
// holds D[i = (l >> 4) + 4 r][j = l & 15].  Here A = W (rows: replicates, k: patterns) and
// B = s^T (k: patterns, columns: trees): BOTH operands are contiguous along p in memory while
// the instruction wants lanes that stride across rows.  So a workgroup (four waves) reads a
// 64 x 32 block of each -- 16 bytes per lane along p, 16 lanes per 256-byte row piece --,
// keeps it in LDS row by row and reads the operands back column-wise.  The LDS row stride is 34
// doubles: 16-byte aligned for the staging writes, and the 32 lanes of half a wave (16 rows x 2
// patterns) then read 64 different banks.
//
// A wave owns a 32 x 32 block of C: four 16 x 16 accumulators, four matrix instructions per two
// operand reads of each side.  The next block of both operands is fetched into registers while
// the current one is multiplied.
//
// Order of summation: every C[b][t] has ONE accumulator that takes the patterns in ascending
// order, four per instruction, from p = 0.  Nothing about it depends on B, T, the block the pair
// falls in or the launch size; there is no split along p.  The tails (p >= P, b >= B, t >= T) are
// zeros in BOTH operands, read through a clamped index: padding adds +0 and can make no NaN.
#include <hip/hip_runtime.h>

#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {

typedef double double4v __attribute__((ext_vector_type(4)));
typedef double double2v __attribute__((ext_vector_type(2)));

constexpr int kRellBlock = 64;    // rows of W and rows of s per workgroup
constexpr int kRellChunk = 32;    // patterns per LDS block
constexpr int kRellStride = 34;   // LDS row stride in doubles (see above)
constexpr int kRellThreads = 256;
constexpr int kRellLoads = kRellBlock * kRellChunk / 2 / kRellThreads;  // 16-byte pieces per thread and operand: 4

// Two consecutive patterns (p, p + 1; p even) of row `row` of a [rows][P] matrix; zeros beyond
// either end.  VEC: P is even and the matrix is 16-byte aligned, so the pair is one aligned
// 16-byte load that is inside the row or wholly outside it.
template <bool VEC>
__device__ __forceinline__ double2v rell_fetch(const double* __restrict__ m, int rows, int P, int row, int p) {
  const bool row_ok = row < rows;
  const size_t base = (size_t)(row_ok ? row : 0) * P;
  double2v v;
  if (VEC) {
    const bool ok = row_ok && p < P;
    v = *reinterpret_cast<const double2v*>(m + base + (ok ? p : 0));
    if (!ok) v = double2v{0.0, 0.0};
  } else {
    const bool ok0 = row_ok && p < P, ok1 = row_ok && p + 1 < P;
    const double x0 = m[base + (ok0 ? p : 0)], x1 = m[base + (ok1 ? p + 1 : 0)];
    v = double2v{ok0 ? x0 : 0.0, ok1 ? x1 : 0.0};
  }
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(kRellThreads) void rell_product_kernel(RellArgs a) {
  __shared__ double w_l[kRellBlock * kRellStride];
  __shared__ double s_l[kRellBlock * kRellStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.y * kRellBlock, t0 = blockIdx.x * kRellBlock;
  const int B = a.B, T = a.T, P = a.P;
  // staging: piece q of this thread is row 16 q + (tid >> 4), patterns 2 (tid & 15), + 1
  const int st_row = tid >> 4, st_p = 2 * (tid & 15);
  double2v wr[kRellLoads], sr[kRellLoads];
  auto fetch = [&](int p0) {
#pragma unroll
    for (int q = 0; q < kRellLoads; q++) {
      wr[q] = rell_fetch<VEC>(a.weights, B, P, b0 + 16 * q + st_row, p0 + st_p);
      sr[q] = rell_fetch<VEC>(a.pattern_ll, T, P, t0 + 16 * q + st_row, p0 + st_p);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < kRellLoads; q++) {
      const int at = (16 * q + st_row) * kRellStride + st_p;
      *reinterpret_cast<double2v*>(w_l + at) = wr[q];
      *reinterpret_cast<double2v*>(s_l + at) = sr[q];
    }
  };
  // this wave's 32 x 32 block of the workgroup's 64 x 64, and this lane's operand element
  const int wb = (wave >> 1) * 32, wt = (wave & 1) * 32;
  const int oi = lane & 15, ok = lane >> 4;
  const double* wa = w_l + (wb + oi) * kRellStride + ok;
  const double* sa = s_l + (wt + oi) * kRellStride + ok;
  double4v acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = double4v{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  for (int p0 = 0; p0 < P; p0 += kRellChunk) {
    __syncthreads();  // the block before this one has been read
    stage();
    __syncthreads();
    if (p0 + kRellChunk < P) fetch(p0 + kRellChunk);  // in flight under the products below
#pragma unroll
    for (int k = 0; k < kRellChunk; k += 4) {
      const double a0 = wa[k], a1 = wa[16 * kRellStride + k];
      const double c0 = sa[k], c1 = sa[16 * kRellStride + k];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c1, acc[1][1], 0, 0, 0);
    }
  }
  // D[i = (lane >> 4) + 4 r][j = lane & 15]: 16 lanes write 128 consecutive bytes of a row of C
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int b = b0 + wb + 16 * i + (lane >> 4) + 4 * r, t = t0 + wt + 16 * j + (lane & 15);
        if (b < B && t < T) a.c[(size_t)b * T + t] = acc[i][j][r];
      }
}

// Row pass: a wave per replicate.  Lane l takes trees l, l + 64, ... in ascending order; the
// lanes are combined by a fixed butterfly.  (maximum, lowest index among equals) is an
// associative, commutative choice, so every lane ends with the same pair.
__global__ __launch_bounds__(256) void rell_rows_kernel(RellArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int T = a.T;
  const double* __restrict__ row = a.c + (size_t)b * T;
  constexpr int kNone = 0x7fffffff;  // this lane has seen no tree
  double m = -__builtin_inf();
  int best = kNone;
  for (int t = lane; t < T; t += 64) {
    const double v = row[t];
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
  double den = 0.0;
  for (int t = lane; t < T; t += 64) den += exp(row[t] - m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) den += __shfl_xor(den, off, 64);  // (both partners add the same two values: one order)
  if (lane == 0) {
    a.row_max[b] = m;
    a.row_inv[b] = 1.0 / den;
    if (a.best) a.best[b] = best;
    atomicAdd(a.counts + best, 1);  // integer
  }
}

// Column pass: a lane per tree, replicates in ascending order (coalesced across trees, ordered
// along b: reproducible).
__global__ __launch_bounds__(64) void rell_columns_kernel(RellArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= a.T) return;
  a.bp[t] = (double)a.counts[t] / (double)a.B;
  if (!a.elw) return;
  double sum = 0.0;
  const double* __restrict__ c = a.c + t;
#pragma unroll 8
  for (int b = 0; b < a.B; b++) sum += exp(c[(size_t)b * a.T] - a.row_max[b]) * a.row_inv[b];
  a.elw[t] = sum / (double)a.B;
}

// Mixture marginal: a lane per pattern; the maximum first, then the trees in ascending order.
// (uniform weights, log_weights == nullptr: m + log(sum / T) -- T equal rows give the row back)
__global__ __launch_bounds__(256) void mixture_patterns_kernel(MixtureArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.P) return;
  const double* __restrict__ s = a.pattern_ll + p;
  double m = -__builtin_inf();
  for (int t = 0; t < a.T; t++) {
    const double v = s[(size_t)t * a.P] + (a.log_weights ? a.log_weights[t] : 0.0);
    m = v > m ? v : m;
  }
  double out = m;
  if (m > -__builtin_inf()) {
    double sum = 0.0;
    for (int t = 0; t < a.T; t++)
      sum += exp(s[(size_t)t * a.P] + (a.log_weights ? a.log_weights[t] : 0.0) - m);
    out = m + log(a.log_weights ? sum : sum / (double)a.T);
  }
  a.out_pattern[p] = out;
}
// ... and the weighted sum over the patterns: one workgroup, thread i takes patterns i, i + 256,
// ... in ascending order, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(256) void mixture_sum_kernel(MixtureArgs a) {
  __shared__ double part[256];
  double sum = 0.0;
  for (int p = threadIdx.x; p < a.P; p += 256) sum += a.pattern_weights[p] * a.out_pattern[p];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.out_total[0] = part[0];
}

// Patterns without information: every tip vector all ones (an all-gap column).  A lane per pattern.
__global__ __launch_bounds__(256) void pattern_blank_kernel(const uint8_t* masks, const double* partials, int n, int P,
                                                            uint8_t* blank) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  bool all = true;
  for (int x = 0; x < n; x++) {
    const size_t i = (size_t)x * P + p;
    if (masks) all = all && masks[i] == 0xF;
    else all = all && partials[4 * i] == 1.0 && partials[4 * i + 1] == 1.0 && partials[4 * i + 2] == 1.0 && partials[4 * i + 3] == 1.0;
  }
  blank[p] = all ? 1 : 0;
}

}  // namespace

void launch_pattern_blank(const uint8_t* masks, const double* partials, int n, int P, uint8_t* blank, hipStream_t s) {
  hipLaunchKernelGGL(pattern_blank_kernel, dim3((P + 255) / 256), dim3(256), 0, s, masks, partials, n, P, blank);
}

const char* rell_product_kernel_name() { return "rell_product_kernel"; }

void launch_rell(const RellArgs& a, hipStream_t s) {
  const dim3 grid((a.T + kRellBlock - 1) / kRellBlock, (a.B + kRellBlock - 1) / kRellBlock);
  const bool vec = a.P % 2 == 0 && (reinterpret_cast<uintptr_t>(a.weights) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.pattern_ll) & 15) == 0;
  if (vec) hipLaunchKernelGGL(rell_product_kernel<true>, grid, dim3(kRellThreads), 0, s, a);
  else hipLaunchKernelGGL(rell_product_kernel<false>, grid, dim3(kRellThreads), 0, s, a);
  hipLaunchKernelGGL(rell_rows_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(rell_columns_kernel, dim3((a.T + 63) / 64), dim3(64), 0, s, a);
}

void launch_pattern_mixture(const MixtureArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(mixture_patterns_kernel, dim3((a.P + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(mixture_sum_kernel, dim3(1), dim3(256), 0, s, a);
}

}  // namespace miphylo
