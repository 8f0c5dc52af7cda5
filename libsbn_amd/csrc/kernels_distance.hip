// Pairwise maximum-likelihood distances from the engine's alignment (gfx950 /
// CDNA4, wave64): the 4 x 4 substitution-count matrices of all pairs of taxa for B sets of
// pattern weights, and the distance that maximises each pair's likelihood.
//
//   N_r[i][j][a][b] = sum_p W[r][p] [tip_i(p) = a] [tip_j(p) = b]   =   (X diag(w_r) X^T)[4i+a][4j+b]
//
// X is the one-hot [4n][P] form of the alignment.  The product runs on v_mfma_f64_16x16x4_f64
// (operand maps: header of kernels_aa.hip): lane l holds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15]; a 16-row operand tile is four taxa x four states, k is the pattern.
// Both operands are formed in registers from one-byte tip codes (0..3: the state, 4: missing --
// distance_codes_kernel, once per engine): A = the replicate's weight where the row taxon shows
// the lane's state, else 0; B = 1 or 0 likewise.  Register r of the result holds
// D[i = (l >> 4) + 4 r][j = l & 15]: r is the taxon within the row tile, the lanes are
// 16 x state a + 4 x taxon_j + state b -- the 16 counts of a pair sit in one register.
//
// A wave owns one 16 x 16 tile block (four taxa by four taxa, on or above the diagonal) for RW
// replicates that share the B operand.  It reads 16 patterns of its lane's two taxa as one
// 16-byte load each; instruction q of the four that follow takes byte 4 q + k.
//
// Order of summation: every count has ONE accumulator that takes the patterns in ascending
// order, four per instruction, from p = 0.  Nothing about it depends on B, n, RW or where the
// pair falls in the launch.  The tails (p >= P, taxa >= n) are code 4: zeros in BOTH operands;
// the A operand's weight is selected, never multiplied, so whatever is read for a padding
// pattern adds +0.  (Inside the instruction a weight still meets the 0.0 of taxon j's other
// states: the weights must be finite, as the header says -- an infinite one makes NaN counts
// for the pairs of the taxa that show a state at its pattern.)  With integer weights every
// partial sum is an exact integer.
//
// The distances are a second kernel over the counts, a thread per (replicate, pair): no
// cross-thread arithmetic, so equal counts give bit-identical distances.
#include <hip/hip_runtime.h>

#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {

typedef double double4v __attribute__((ext_vector_type(4)));

// Tip codes [n4][Pp] (n4: n rounded up to whole tiles of four taxa, Pp: P rounded up to 16):
// the compact state, or -- an engine made from tip partials -- the state whose unit vector the
// tip's vector is exactly; everything else, and the padding, is 4.
__global__ __launch_bounds__(256) void distance_codes_kernel(const int8_t* states, const double* partials, int n,
                                                             int P, int n4, int Pp, uint8_t* codes) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n4 * Pp) return;
  const int x = (int)(idx / Pp), p = (int)(idx % Pp);
  int code = 4;
  if (x < n && p < P) {
    const size_t i = (size_t)x * P + p;
    if (partials) {
      int ones = 0, zeros = 0, last = 0;
      for (int s = 0; s < 4; s++) {
        const double v = partials[4 * i + s];
        if (v == 1.0) {
          ones++;
          last = s;
        } else if (v == 0.0) {
          zeros++;
        }
      }
      if (ones == 1 && zeros == 3) code = last;
    } else {
      const int s = states[i];
      if (s >= 0 && s < 4) code = s;
    }
  }
  codes[idx] = (uint8_t)code;
}

__device__ __forceinline__ unsigned word_of(const uint4& v, int q) {
  return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
}

// tile block `tb` of the upper triangle (rows of nt, nt - 1, ... blocks) -> (ti, tj), ti <= tj
__device__ __forceinline__ void tile_block(int tb, int nt, int& ti, int& tj) {
  int i = 0;
  while (tb >= nt - i) {
    tb -= nt - i;
    i++;
  }
  ti = i;
  tj = i + tb;
}

template <int RW>
__global__ __launch_bounds__(256) void pair_counts_kernel(DistanceArgs a) {
  const int lane = threadIdx.x & 63;
  const int groups = (a.B + RW - 1) / RW;
  const int nt = a.n4 >> 2;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // (wave-uniform)
  if (item >= (long)groups * (nt * (nt + 1) / 2)) return;
  const int rg = (int)(item % groups);
  int ti, tj;
  tile_block((int)(item / groups), nt, ti, tj);
  const int k = lane >> 4, state = lane & 3, tx = (lane & 15) >> 2;
  const int P = a.P, Pp = a.Pp;
  const uint8_t* __restrict__ row_a = a.codes + (size_t)(4 * ti + tx) * Pp;
  const uint8_t* __restrict__ row_b = a.codes + (size_t)(4 * tj + tx) * Pp;
  const double* w[RW];
#pragma unroll
  for (int r = 0; r < RW; r++) {
    const int rep = rg * RW + r;
    w[r] = a.weights + (size_t)(rep < a.B ? rep : a.B - 1) * P;  // (a replicate past the end: read, never stored)
  }
  double4v acc[RW];
#pragma unroll
  for (int r = 0; r < RW; r++) acc[r] = double4v{0.0, 0.0, 0.0, 0.0};

  for (int p0 = 0; p0 < Pp; p0 += 16) {
    const uint4 ca = *reinterpret_cast<const uint4*>(row_a + p0);
    const uint4 cb = *reinterpret_cast<const uint4*>(row_b + p0);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int p = p0 + 4 * q + k;
      const int pc = p < P ? p : P - 1;
      const bool hit_a = (int)((word_of(ca, q) >> (8 * k)) & 0xff) == state;
      const double b = (int)((word_of(cb, q) >> (8 * k)) & 0xff) == state ? 1.0 : 0.0;
#pragma unroll
      for (int r = 0; r < RW; r++) {
        const double wv = w[r][pc];
        acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(hit_a ? wv : 0.0, b, acc[r], 0, 0, 0);
      }
    }
  }
  // register r: taxon 4 ti + r; lane: state a = lane >> 4, taxon 4 tj + tx, state b
  const int n = a.n;
  const size_t pairs = (size_t)n * (n - 1) / 2;
  const int j = 4 * tj + tx;
#pragma unroll
  for (int r = 0; r < RW; r++) {
    const int rep = rg * RW + r;
    if (rep >= a.B) continue;
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const int i = 4 * ti + x;
      if (i < j && j < n) {
        const size_t pair = (size_t)i * n - (size_t)i * (i + 1) / 2 + (j - i - 1);
        a.counts[((size_t)rep * pairs + pair) * 16 + (lane >> 4) * 4 + state] = acc[r][x];
      }
    }
  }
}

// ------------------------------------------------------------------------
// The distance of one pair from its counts:
//   l(t) = sum_ab N[a][b] log L_ab(t),   L_ab(t) = sum_k c_k P_ab(r_k t)
// With P(t) = I + V diag(expm1(lambda t)) V^-1 (the form of transition_kernel) and
// C[ab][x] = V[a][x] V^-1[x][b]:  L_ab = [a = b] + sum_x C[ab][x] E0[x], its derivatives the same
// sums over E1, E2, where E_m[x] = sum_k c_k (lambda_x r_k)^m exp(lambda_x r_k t) (m = 0: expm1).
// ------------------------------------------------------------------------
struct PairModel {
  const double *C, *lam, *rate, *cw;  // LDS
  int K;
};

__device__ __forceinline__ void pair_derivatives(const PairModel& m, const double* N, double t, double& g,
                                                 double& h) {
  double E0[4] = {0, 0, 0, 0}, E1[4] = {0, 0, 0, 0}, E2[4] = {0, 0, 0, 0};
  for (int k = 0; k < m.K; k++) {
    const double r = m.rate[k], c = m.cw[k];
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const double l = m.lam[x] * r;
      const double em = expm1(l * t);
      const double ce = c * (em + 1.0);
      E0[x] += c * em;
      E1[x] += l * ce;
      E2[x] += l * l * ce;
    }
  }
  g = 0.0;
  h = 0.0;
#pragma unroll
  for (int ab = 0; ab < 16; ab++) {
    const double* C = m.C + 4 * ab;
    const double L = ((ab >> 2) == (ab & 3) ? 1.0 : 0.0) + (C[0] * E0[0] + C[1] * E0[1] + C[2] * E0[2] + C[3] * E0[3]);
    const double L1 = C[0] * E1[0] + C[1] * E1[1] + C[2] * E1[2] + C[3] * E1[3];
    const double L2 = C[0] * E2[0] + C[1] * E2[1] + C[2] * E2[2] + C[3] * E2[3];
    if (N[ab] != 0.0) {  // (a count of zero adds nothing, whatever L is)
      const double q = L1 / L;
      g += N[ab] * q;
      h += N[ab] * (L2 / L - q * q);
    }
  }
}

// status: 0 converged, 1 on the lower bound, 2 on the upper bound, 3 no data, 4 iteration limit
__device__ __forceinline__ double pair_distance(const PairModel& m, const double* N, double tmin, double tmax,
                                                double tol, int max_iter, int& status) {
  double total = 0.0, same = 0.0;
#pragma unroll
  for (int ab = 0; ab < 16; ab++) {
    total += N[ab];
    if ((ab >> 2) == (ab & 3)) same += N[ab];
  }
  if (!(total > 0.0)) {
    status = 3;
    return tmax;
  }
  double g, h;
  pair_derivatives(m, N, tmin, g, h);
  if (!(g > 0.0)) {
    status = 1;
    return tmin;
  }
  pair_derivatives(m, N, tmax, g, h);
  if (!(g < 0.0)) {
    status = 2;
    return tmax;
  }
  // the JC69 closed form of the mismatch share, clamped into the box
  const double share = 1.0 - same / total;
  double t = share < 0.75 ? -0.75 * log(1.0 - share * (4.0 / 3.0)) : tmax;
  t = fmin(fmax(t, tmin), tmax);
  double lo = tmin, hi = tmax;  // l' > 0 at lo, < 0 at hi
  status = 4;
  for (int it = 0; it < max_iter; it++) {
    pair_derivatives(m, N, t, g, h);
    if (g > 0.0) lo = t;
    else if (g < 0.0) hi = t;
    // (a step that lands ON an end of the bracket has not left it: l' at a point next to the
    // maximum is rounding noise of either sign, and the step from there is no step at all)
    double next = h < 0.0 ? t - g / h : hi + 1.0;
    if (!(next >= lo && next <= hi)) next = 0.5 * (lo + hi);
    if (g == 0.0) next = t;
    const double step = next - t;
    t = next;
    if (fabs(step) <= tol * fmax(t, 1e-3)) {
      status = 0;
      break;
    }
  }
  return t;
}

__global__ __launch_bounds__(256) void pair_distance_kernel(DistanceArgs a) {
  __shared__ double sC[64], sLam[4], sRate[kMaxCategories], sCw[kMaxCategories];
  const DevModel& dm = *a.model;
  if (threadIdx.x < 64) {
    const int ab = threadIdx.x >> 2, x = threadIdx.x & 3;
    sC[threadIdx.x] = dm.V[(ab >> 2) * 4 + x] * dm.Vinv[x * 4 + (ab & 3)];
  }
  if (threadIdx.x < 4) sLam[threadIdx.x] = dm.lambda[threadIdx.x];
  if ((int)threadIdx.x < a.K) {
    sRate[threadIdx.x] = dm.cat_rate[threadIdx.x];
    sCw[threadIdx.x] = dm.cat_weight[threadIdx.x];
  }
  __syncthreads();
  const int n = a.n, rep = blockIdx.y;
  const long pairs = (long)n * (n - 1) / 2;
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  double* dist = a.out_dist + (size_t)rep * n * n;
  if (item >= pairs) {
    if (item < pairs + n) dist[(item - pairs) * (n + 1)] = 0.0;  // the diagonal
    return;
  }
  // pair -> (i, j): the row whose first pair is the last one not after `item`
  const double m2 = 2.0 * n - 1.0;
  int i = (int)((m2 - sqrt(m2 * m2 - 8.0 * (double)item)) * 0.5);
  i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
  while (i > 0 && (long)i * n - (long)i * (i + 1) / 2 > item) i--;
  while (i < n - 2 && (long)(i + 1) * n - (long)(i + 1) * (i + 2) / 2 <= item) i++;
  const int j = i + 1 + (int)(item - ((long)i * n - (long)i * (i + 1) / 2));
  const double* src = a.counts + ((size_t)rep * pairs + item) * 16;
  double N[16];
#pragma unroll
  for (int q = 0; q < 16; q++) N[q] = src[q];
  if (a.out_counts) {
    double* dst = a.out_counts + ((size_t)rep * pairs + item) * 16;
#pragma unroll
    for (int q = 0; q < 16; q++) dst[q] = N[q];
  }
  const PairModel m{sC, sLam, sRate, sCw, a.K};
  int status;
  const double d = pair_distance(m, N, a.tmin, a.tmax, a.tol, a.max_iter, status);
  dist[(size_t)i * n + j] = d;
  dist[(size_t)j * n + i] = d;
  if (a.out_status) a.out_status[(size_t)rep * pairs + item] = (int8_t)status;
}

}  // namespace

void launch_distance_codes(const int8_t* states, const double* partials, int n, int P, uint8_t* codes,
                           hipStream_t s) {
  const int n4 = distance_code_rows(n), Pp = distance_code_stride(P);
  const size_t total = (size_t)n4 * Pp;
  hipLaunchKernelGGL(distance_codes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, states,
                     partials, n, P, n4, Pp, codes);
}

const char* pair_counts_kernel_name() { return "pair_counts_kernel"; }

void launch_pair_distances(const DistanceArgs& a, hipStream_t s) {
  const long nt = a.n4 / 4, blocks = nt * (nt + 1) / 2;
  // (few replicates: a wave per replicate; else four share the column operand)
  if (a.B < 4) {
    const long items = blocks * a.B;
    hipLaunchKernelGGL(pair_counts_kernel<1>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, a);
  } else {
    const long items = blocks * ((a.B + 3) / 4);
    hipLaunchKernelGGL(pair_counts_kernel<4>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, a);
  }
  const long per = (long)a.n * (a.n - 1) / 2 + a.n;
  hipLaunchKernelGGL(pair_distance_kernel, dim3((unsigned)((per + 255) / 256), a.B), dim3(256), 0, s, a);
}

}  // namespace miphylo
