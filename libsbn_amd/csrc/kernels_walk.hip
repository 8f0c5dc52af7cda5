// The matrix-core gradient walk, second generation (round 3): gradient_walk_kernel -- the walk
// itself is gradient_walk_body (mi_phylo_walk2_device.h), here with HESS = false --,
// transition_macro_kernel, which writes the matrices in the order the walk consumes them, and
// the rules that choose where a call's stored vectors live (LDS or the arena).
#include <hip/hip_runtime.h>

namespace miphylo {
#ifdef MI_WALK_TIMELINE
// diagnostic build (make timeline; tools/walk_timeline.py): eight words per wave, written at
// the end of gradient_walk_body
__device__ long long g_walk_timeline[65536 * 8];
#endif
}  // namespace miphylo

#include "mi_phylo_walk2_device.h"

namespace miphylo {

namespace {

template <int R, bool RESCALE, bool SUBST, bool ARENA, bool COMPACT>
__global__ __launch_bounds__(kTile, 2) void gradient_walk_kernel(LikArgs a) {
  gradient_walk_body<R, RESCALE, SUBST, ARENA, COMPACT, false>(a);
}

// ------------------------------------------------------------------------
// Transition matrices in the order the walk consumes them.  One thread per (gradient
// evaluation, macro, position, category): P = I + V expm1(L r t) V^-1 of the position's
// node (DESIGN.md "Accuracy"; negative entries clamped as BEAGLE does) and the matrix of the
// pre-order step -- P^T for an internal edge, P Q for a tip edge -- interleaved {f, tr} per
// lane slot (lo, hi): f = P[lo][hi], tr = P[hi][lo] | (P Q)[lo][hi].  Staged through LDS so
// that a block writes whole cache lines.  SUBST: the divided differences Phi[hi][lo] too.
// ------------------------------------------------------------------------
constexpr int kTmBlock = 128;
__global__ __launch_bounds__(kTmBlock) void transition_macro_kernel(TransitionMacroArgs a) {
  // One thread per (node, category) of ONE gradient evaluation (blockIdx.x): as many threads
  // as matrices, none idle on positions that do not exist.  Where a node's matrices go -- its
  // (macro, position) -- comes from a map the block builds from the tree's macro entries.
  // The 16-double matrices are staged one per thread (row stride 17: conflict-free) and
  // written out as the f halves, then the tr halves, of the 256-byte records.
  __shared__ double stage[kTmBlock * 17];
  __shared__ int rec_of[kTmBlock];
  extern __shared__ int slot_of[];  // [N - 1]: node -> macro * 6 + position
  const int Mmax = max_macros(a.n), groups = (a.K + 3) / 4;
  const int ge = blockIdx.x;  // gradient evaluation of this launch (grid.x: no 65535 limit)
  int t, mi;
  a.map.decode(a.eval_begin + ge, t, mi);
  const MacroEntry* mac = a.macros + (size_t)t * macro_stride(a.n);
  const int M = a.macro_count[t];
  for (int j = threadIdx.x; j < M * 6; j += kTmBlock) {
    const int m = j / 6, pos = j - m * 6;
    const MacroEntry& me = mac[m];
    if (pos < 2 || ((me.shape >> (2 * ((pos - 2) >> 1))) & 3) == 2)
      slot_of[pos < 2 ? me.child[pos] : me.grand[pos - 2]] = j;
  }
  __syncthreads();
  const int idx = blockIdx.y * kTmBlock + threadIdx.x;  // node * K + category
  const int node = idx / a.K, k = idx - node * a.K;
  const bool live = node < a.N - 1 && M > 0;
  double Pm[16];
  const DevModel& md = a.models[mi];
  bool tip = false;
  double tau = 0;
  if (live) {
    tip = node < a.n;
    tau = md.cat_rate[k] * a.bl_eff[(size_t)t * a.N + node];
    double ex[4], W[16];
    for (int x = 0; x < 4; x++) ex[x] = expm1(md.lambda[x] * tau);
    for (int x = 0; x < 4; x++)
      for (int j = 0; j < 4; j++) W[x * 4 + j] = ex[x] * md.Vinv[x * 4 + j];
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        double sum = i == j ? 1.0 : 0.0;
        for (int x = 0; x < 4; x++) sum += md.V[i * 4 + x] * W[x * 4 + j];
        Pm[i * 4 + j] = sum > 0 ? sum : 0;
        stage[threadIdx.x * 17 + i * 4 + j] = Pm[i * 4 + j];
      }
    const int slot = slot_of[node], m = slot / 6, pos = slot - m * 6;
    // record index: (evaluation, macro, category group, position, category in the group)
    rec_of[threadIdx.x] = ((((ge * Mmax + m) * groups + (k >> 2)) * 6 + pos) << 2) + (k & 3);
  } else {
    rec_of[threadIdx.x] = -1;
  }
  __syncthreads();
  for (int x = threadIdx.x; x < kTmBlock * 16; x += kTmBlock) {
    const int rec = rec_of[x >> 4];
    if (rec >= 0) a.mmats[(size_t)rec * 32 + (x & 15) * 2] = stage[(x >> 4) * 17 + (x & 15)];
  }
  __syncthreads();
  if (live) {
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        double trv;
        if (tip) {
          trv = 0;
          for (int x = 0; x < 4; x++) trv += Pm[i * 4 + x] * md.Q[x * 4 + j];
        } else {
          trv = Pm[j * 4 + i];
        }
        stage[threadIdx.x * 17 + i * 4 + j] = trv;
      }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < kTmBlock * 16; x += kTmBlock) {
    const int rec = rec_of[x >> 4];
    if (rec >= 0) a.mmats[(size_t)rec * 32 + (x & 15) * 2 + 1] = stage[(x >> 4) * 17 + (x & 15)];
  }
  if (a.mphi != nullptr) {
    __syncthreads();
    if (live) {
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)  // slot (lo = i, hi = j) holds Phi[hi][lo]
          stage[threadIdx.x * 17 + i * 4 + j] = phi_divided_difference(md.lambda[j], md.lambda[i], tau);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < kTmBlock * 16; x += kTmBlock) {
      const int rec = rec_of[x >> 4];
      if (rec >= 0) a.mphi[(size_t)rec * 16 + (x & 15)] = stage[(x >> 4) * 17 + (x & 15)];
    }
  }
}

}  // namespace

size_t gradient_walk_lds_bytes_for(int n, int K, bool rescale, bool subst, int slots, int regs) {
  const int kp = K == 1 ? 1 : (K == 2 ? 2 : 4);
  const int R = regs > 0 ? regs : kLlR;
  // (compact tip words for fewer than three categories -- not in the analytic variant)
  const unsigned col = (kp < 4 && !subst) ? kTwColCompact : kTwCol;
  size_t bytes = (size_t)max_macros(n) * (16 / kp) * col + (subst ? 32 : 0) +
                 sizeof(double) * (size_t)slots * R * kTile;
  if (rescale) bytes += ((sizeof(int16_t) * (size_t)max_stored(n) * R * (16 / kp) + 7) / 8) * 8;
  return bytes;
}
size_t gradient_walk_lds_bytes(int n, int K, bool rescale, bool subst, int regs) {
  return gradient_walk_lds_bytes_for(n, K, rescale, subst, max_stored(n), regs);
}
size_t gradient_walk_mats_bytes_per_eval(int n, int K) {
  return (size_t)max_macros(n) * ((K + 3) / 4) * 24 * 32 * sizeof(double);
}

void launch_transition_macro(const TransitionMacroArgs& a, hipStream_t s) {
  if (a.count <= 0) return;
  const int per_eval = (a.N - 1) * a.K;
  const dim3 grid(a.count, (per_eval + kTmBlock - 1) / kTmBlock);
  hipLaunchKernelGGL(transition_macro_kernel, grid, dim3(kTmBlock), sizeof(int) * (size_t)(a.N - 1), s, a);
}

template <bool RESCALE, bool SUBST, bool ARENA, bool COMPACT>
static void launch_walk_variant(const LikArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  allow_large_lds(reinterpret_cast<const void*>(gradient_walk_kernel<kLlR, RESCALE, SUBST, ARENA, COMPACT>), lds);
  hipLaunchKernelGGL((gradient_walk_kernel<kLlR, RESCALE, SUBST, ARENA, COMPACT>), grid, dim3(kTile), lds, s, a);
}
template <bool ARENA>
static void launch_walk_store(const LikArgs& a, dim3 grid, size_t lds, bool rescale, bool subst,
                              hipStream_t s) {
  const bool compact = a.kp < 4 && !subst;  // (as gradient_walk_lds_bytes_for sizes the tip words)
  if (rescale && subst) launch_walk_variant<true, true, ARENA, false>(a, grid, lds, s);
  else if (subst) launch_walk_variant<false, true, ARENA, false>(a, grid, lds, s);
  else if (rescale && compact) launch_walk_variant<true, false, ARENA, true>(a, grid, lds, s);
  else if (rescale) launch_walk_variant<true, false, ARENA, false>(a, grid, lds, s);
  else if (compact) launch_walk_variant<false, false, ARENA, true>(a, grid, lds, s);
  else launch_walk_variant<false, false, ARENA, false>(a, grid, lds, s);
}
void launch_gradient_walk(const LikArgs& a_in, int count, bool rescale, bool subst, const Switches& sw,
                          hipStream_t s) {
  if (count <= 0) return;
  LikArgs a = a_in;
  a.kp = a.K == 1 ? 1 : (a.K == 2 ? 2 : 4);
  a.cat_groups = gradient_mfma_groups(a.K);
  // Jobs.  The launch's first `big` evaluations (a multiple of 8: whole XCD groups) are
  // walked by waves that take `tpw` pattern tiles each, one after the other (what belongs to
  // the tree stays in registers, the next tile's tip bytes arrive during the current walk, no
  // wave slot stands empty in between: -6 % per 1000 DS1 trees); the evaluations after them
  // get a wave per tile.  Workgroups start in id order, so the small jobs come last and level
  // out the end of the launch: the slots finish their big jobs up to one big job apart, which
  // takes about (tpw / 2 + 1) rounds of small jobs to fill.  tpw maximises the share of the
  // work that runs as the second or later tile of a wave.  (A wave stays in one category
  // group; the arena and analytic variants take one tile per wave: kernel comment.)
  // MI_PHYLO_WALK_TILES_PER_WAVE=k forces k (1: every tile its own wave, as until round 3).
  const int forced_tpw = sw.walk_tiles_per_wave;
  const int gtiles = gradient_mfma_tiles(a.P, a.K) * a.cat_groups;
  const bool arena_variant =
      a.store ? a.store == 2
              : gradient_walk_use_arena(sw.gradient_store, a.n, a.K, rescale, subst, (size_t)gtiles * (size_t)count);
  int tpw = 1, big = 0;
  if (a.cat_groups == 1 && !arena_variant && !subst) {
    const double slots = (double)device_compute_units() * gradient_walk_waves_per_cu(sw.gradient_store, a.n, a.K);
    double best = 0;
    for (int k = forced_tpw ? forced_tpw : 2; k <= (forced_tpw ? forced_tpw : 8); k++) {
      // (measured, 1000 and 125 DS1 trees: fewer small jobs -- k / 4 + 1, k / 8 + 1/2 rounds --
      // lose more at the end of the launch than the larger share of big jobs gains)
      const int small = (int)std::ceil((0.5 * k + 1.0) * slots / gtiles);
      const int b = small < count ? (count - small) & ~7 : 0;
      const double gain = (double)b / count * (1.0 - 1.0 / k);
      if (gain > best) {
        best = gain;
        tpw = k;
        big = b;
      }
    }
  }
  a.walk_evals = count;
  a.walk_groups = (gtiles + tpw - 1) / tpw;
  a.walk_big_evals = big;
  const dim3 grid((unsigned)((size_t)a.walk_big_evals * a.walk_groups +
                             (size_t)(count - a.walk_big_evals) * gtiles));
  if (arena_variant) {
    launch_walk_arena_ladder(a, grid.x, rescale, subst, [&](const LikArgs& part, size_t lds) {
      launch_walk_store<true>(part, grid, lds, rescale, subst, s);
    });
    return;
  }
  launch_walk_store<false>(a, grid, gradient_walk_lds_bytes(a.n, a.K, rescale, subst), rescale,
                           subst, s);
}

bool gradient_walk_use_arena(int store, int n, int K, bool rescale, bool subst, size_t waves, bool lut, int regs) {
  const int forced = store;  // MI_PHYLO_GRADIENT_STORE: 0 unset, 1 lds, 2 arena
  if (regs > kLlR) {
    // A wide-tile engine (look-up walk, kernels_walk3.hip): wide tiles pay in the arena; the form
    // with every vector in LDS runs at one wave per SIMD (registers) and takes the calls whose
    // waves are all resident at once at that occupancy -- 16 trees of 45 taxa x 200 patterns
    // 0.052 (default tiles in LDS) / 0.068 ms (wide, arena) before it existed.  The tile width
    // never depends on the call: a tree's outputs do not depend on the batch it came in.
    const size_t lds_w = gradient_walk_lds_bytes(n, K, rescale, subst, regs);
    const bool fits = lds_w <= 160 * 1024;
    if (forced == 1 && fits) return false;
    if (forced == 2 || !fits) return true;
    const size_t per_cu = std::min<size_t>(4, (160 * 1024) / lds_w);
    return waves > (size_t)device_compute_units() * per_cu;
  }
  const size_t lds_all = gradient_walk_lds_bytes(n, K, rescale, subst);
  const bool lds_fits = lds_all <= 160 * 1024;
  if (forced == 1 && lds_fits) return false;
  if (forced == 2) return true;
  if (lds_fits && arena_single_launch(lds_all, waves)) return false;  // a call of a few trees
  // (round 5, tools/audit_paths.py with the store forced either way: with five and six waves per
  // CU the LDS store still wins -- 31 taxa x 1000 patterns x 4 categories 1.29 against 1.54 ms per
  // 1000 trees, 36 x 200: 0.41 / 0.46, one category 0.36 / 0.41 -- and from four waves down the
  // arena does; the round-1 cross-over "fewer than seven" dated from the first generation)
  // (round 6: the look-up walk's arena variant -- stored vectors back from the arena in 16-byte
  // accesses, requested with the operands -- wins one step earlier: at five waves per CU the
  // arena's eight take 36 taxa x 1812 patterns in 2.68 against 2.87 ms per 1000 trees, 41 x 1137
  // in 1.96 against 2.07; at six -- 29 to 35 taxa -- the LDS store keeps 1.21 against 1.38)
  return !lds_fits || (160 * 1024) / lds_all < (lut ? 6 : 5);
}
// the same rule for a large batch with no store forced: does this engine's tree size take the arena?
bool gradient_walk_batches_take_arena(int n, int K, bool lut) {
  const size_t lds_all = gradient_walk_lds_bytes(n, K, false, false);
  return lds_all > 160 * 1024 || (160 * 1024) / lds_all < (size_t)(lut ? 6 : 5);
}
int gradient_walk_waves_per_cu(int store, int n, int K);
bool gradient_walk_fits(int n, int K, bool rescale) {
  if (n < 3 || K > kMaxCategories) return false;
  if (gradient_walk_lds_bytes(n, K, rescale, true) <= 160 * 1024) return true;
  return gradient_walk_lds_bytes_for(n, K, rescale, true, gradient_arena_slots_sure(n)) <= 160 * 1024;
}
// waves per CU the kernel's LDS footprint allows (the registers allow 8)
int gradient_walk_waves_per_cu(int store, int n, int K) {
  const size_t lds = gradient_walk_use_arena(store, n, K, false, false, (size_t)-1, false)
                         ? gradient_walk_lds_bytes_for(n, K, false, false, gradient_arena_slots_usual(n))
                         : gradient_walk_lds_bytes(n, K, false, false);
  return (int)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lds, 1));
}
const char* gradient_walk_kernel_name() { return "gradient_walk_kernel"; }

}  // namespace miphylo

#ifdef MI_WALK_TIMELINE
extern "C" __attribute__((visibility("default"))) int mi_debug_walk_timeline(long long* out, int waves) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(miphylo::g_walk_timeline), (size_t)waves * 64);
}
#endif
