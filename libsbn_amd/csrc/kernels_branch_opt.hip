// Maximum-likelihood branch lengths on the device (mi_engine_optimize_branch_lengths_unrooted,
// DESIGN.md 4.9): the per-tree step between two Hessian passes, and the packing of the trees
// that are still active.  (gfx950 / CDNA4, wave64.)  The likelihood work is the Hessian call's
// (kernels_walk_hess.hip, kernels_gradient.hip); nothing here waits on another wave.
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {
using namespace dev;

constexpr int kStepWaves = 4;  // trees per workgroup of the step kernels
// A trial point is accepted when its log-likelihood has not fallen by more than the rounding
// error of a log-likelihood: 2^-48 |logL| (32 units in the last place; the engine's logL is a
// sum over ~1000 patterns and differs from the oracle's by up to 8e-15 relative).  Without it
// the last steps before convergence, whose true gain (g t)^2 / (2 c t^2) ~ 1e-12 is below that
// error, are rejected at random until the step scale underflows (1 of 64 DS1 trees stalled).
constexpr double kLogLikRounding = 0x1p-48;

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double clamp_length(double t, double lo, double hi) {
  return fmin(fmax(t, lo), hi);  // (a NaN becomes lo)
}

// The first trial point: the caller's start clamped into the box.  The entry of the fixed node
// (2n-3) carries no branch and is copied through.  A wave per tree.
__global__ __launch_bounds__(64 * kStepWaves) void branch_opt_init_kernel(BranchOptArgs a, const double* start) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * kStepWaves + (threadIdx.x >> 6);
  if (t >= a.T) return;
  const int nb = a.N - 2;  // branches; a row of lengths has nb + 1 entries
  const size_t row = (size_t)t * (nb + 1);
  for (int j = lane; j <= nb; j += 64) {
    const double s = start[row + j];
    const double x = j < nb ? clamp_length(s, a.tmin, a.tmax) : s;
    a.trial[row + j] = x;
    if (a.trial_full) a.trial_full[row + j] = x;
    a.bl[row + j] = x;
  }
  if (lane == 0) {
    a.ll[t] = -INFINITY;
    a.alpha[t] = 1.0;
    a.evals[t] = 0;
    a.status[t] = kBranchOptActive;
  }
}

// One step of one tree (a wave per packed tree, lanes over branches): accept or reject the
// trial point the Hessian pass has just evaluated, test convergence at the accepted point,
// write the next trial point.  A tree that has left the active set is not touched again.
__global__ __launch_bounds__(64 * kStepWaves) void branch_opt_step_kernel(BranchOptArgs a) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * kStepWaves + (threadIdx.x >> 6);
  if (p >= a.count) return;
  const int t = a.map ? a.map[p] : p;
  if (a.status[t] != kBranchOptActive) return;  // (wave-uniform)
  const int N = a.N, nb = N - 2;
  const int ev = a.evals[t] + 1;
  const double ll_new = a.tr_ll[p];
  const double ll_old = a.ll[t];
  const bool accept = ev == 1 || ll_new >= ll_old - kLogLikRounding * fabs(ll_old);  // (NaN: rejected)
  double alpha = 1.0;
  if (ev > 1) alpha = accept ? fmin(1.0, 2.0 * a.alpha[t]) : 0.5 * a.alpha[t];
  const size_t prow = (size_t)p * (nb + 1), trow = (size_t)t * (nb + 1);
  const size_t pn = (size_t)p * N, tn = (size_t)t * N;
  // the accepted point and its derivatives: the trial's if accepted, else what was kept
  const double* x = accept ? a.trial + prow : a.bl + trow;
  const double* g = accept ? a.tr_g + pn : a.g + tn;
  const double* h = accept ? a.tr_h + pn : a.h + tn;
  const double* s = accept ? a.tr_s + pn : a.s + tn;
  double crit = 0.0;
  for (int j = lane; j < N; j += 64) {
    const double gj = g[j];
    if (accept) {
      a.g[tn + j] = gj;
      a.h[tn + j] = h[j];
      a.s[tn + j] = s[j];
    }
    if (j < nb) {
      const double tj = x[j];
      if (accept) a.bl[trow + j] = tj;
      // projected gradient: 0 where the branch sits on a bound and the gradient points outward
      const bool outward = (tj <= a.tmin && gj < 0.0) || (tj >= a.tmax && gj > 0.0);
      double c = outward ? 0.0 : fabs(gj) * fmax(tj, 1e-3);
      if (c != c) c = INFINITY;  // (fmax would drop a NaN)
      crit = fmax(crit, c);
    }
  }
  crit = wave_max(crit);
  int st = kBranchOptActive;
  if (crit <= a.tol) st = kBranchOptConverged;
  else if (!accept && alpha < 0x1p-20) st = kBranchOptStalled;
  else if (ev >= a.evals_max) st = kBranchOptIterationLimit;
  if (st == kBranchOptActive) {
    for (int j = lane; j < nb; j += 64) {
      const double tj = x[j], gj = g[j], hj = h[j], sj = s[j];
      // curvature: -H where it is safely positive, else the outer-product form S >= 0
      const double c = -hj > 1e-3 * sj ? -hj : sj;
      double d = c > 0.0 ? gj / c : 0.0;
      d = fmin(fmax(d, -0.9 * tj), fmax(4.0 * tj, 0.1));
      const double next = clamp_length(tj + alpha * d, a.tmin, a.tmax);
      a.trial[prow + j] = next;
      if (a.trial_full) a.trial_full[trow + j] = next;
    }
  }
  if (lane == 0) {
    a.evals[t] = ev;
    a.alpha[t] = alpha;
    if (accept) a.ll[t] = ll_new;
    a.status[t] = st;
    if (st == kBranchOptActive) atomicAdd(a.active + a.pass, 1);
  }
}

// Packing, part 1: the active trees of the current packed set, in their order, to the front of
// a new map.  One workgroup walks the set in blocks of 1024 (a ballot per wave, the waves'
// counts through LDS).
__global__ __launch_bounds__(1024) void branch_opt_pack_scan_kernel(int count, const int32_t* map_old,
                                                                     const int32_t* status, int32_t* map_new) {
  __shared__ int wave_count[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int base = 0;
  for (int first = 0; first < count; first += 1024) {
    const int i = first + threadIdx.x;
    const int t = i < count ? (map_old ? map_old[i] : i) : -1;
    const bool on = t >= 0 && status[t] == kBranchOptActive;
    const unsigned long long votes = __ballot(on);
    if (lane == 0) wave_count[wv] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < 16; k++) {
      before += k < wv ? wave_count[k] : 0;
      total += wave_count[k];
    }
    if (on) map_new[base + before + __popcll(votes & ((1ull << lane) - 1ull))] = t;
    base += total;
    __syncthreads();
  }
}
// Packing, part 2: a workgroup per tree of the new set copies its parent ids, its trial
// lengths and its parameter row to the new position.
__global__ __launch_bounds__(64) void branch_opt_pack_gather_kernel(BranchOptPackArgs a) {
  const int p = blockIdx.x, t = a.map[p];
  const int np = a.N - 2, nl = a.N - 1;
  for (int j = threadIdx.x; j < np; j += 64) a.pk_parent[(size_t)p * np + j] = a.parent_ids[(size_t)t * np + j];
  for (int j = threadIdx.x; j < nl; j += 64) a.pk_trial[(size_t)p * nl + j] = a.trial_full[(size_t)t * nl + j];
  for (int j = threadIdx.x; j < a.param_count; j += 64)
    a.pk_params[(size_t)p * a.param_count + j] = a.params[(size_t)t * a.param_count + j];
}

}  // namespace

void launch_branch_opt_init(const BranchOptArgs& a, const double* start, hipStream_t s) {
  hipLaunchKernelGGL(branch_opt_init_kernel, dim3((a.T + kStepWaves - 1) / kStepWaves), dim3(64 * kStepWaves), 0,
                     s, a, start);
}
void launch_branch_opt_step(const BranchOptArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(branch_opt_step_kernel, dim3((a.count + kStepWaves - 1) / kStepWaves),
                     dim3(64 * kStepWaves), 0, s, a);
}
void launch_branch_opt_pack(const BranchOptPackArgs& a, int old_count, const int32_t* map_old,
                            const int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(branch_opt_pack_scan_kernel, dim3(1), dim3(1024), 0, s, old_count, map_old, status,
                     a.map);
  hipLaunchKernelGGL(branch_opt_pack_gather_kernel, dim3(a.count), dim3(64), 0, s, a);
}

}  // namespace miphylo
