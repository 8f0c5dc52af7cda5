// Launch interface between the host engine (mi_phylo_engine.cpp) and the HIP
// kernels (kernels_*.hip).  Plain structs of device pointers.
#pragma once
#include <hip/hip_runtime.h>

#include "mi_phylo_device.h"
#include "mi_phylo_switches.h"

namespace miphylo {

// Evaluations ("virtual trees") of one engine call, numbered
//   [0, T)            main evaluation of tree t with its own model
//   [T, 17T)          GTR gradient only: 16 finite-difference log-likelihoods
//                     per tree (fat_beagle.cpp:400-465), eval T + 16 t + (j-1)
//                     uses model 17 t + j
//   [17T, 18T)        GTR + K>1 gradient only: site-model pass with the model the
//                     reference is left in after the finite differences (j = 16)
struct EvalMap {
  int T;
  int models_per_tree;  // 1, or kFdModels for a GTR gradient call
  __host__ __device__ void decode(int e, int& tree, int& model) const {
    if (e < T) {
      tree = e;
      model = e * models_per_tree;
    } else if (e < 17 * T) {
      tree = (e - T) / 16;
      model = tree * kFdModels + 1 + (e - T) % 16;
    } else {
      tree = e - 17 * T;
      model = tree * kFdModels + 16;
    }
  }
};

struct TreeSetupArgs {
  int n, T, rooted;
  const int32_t* parent_ids;  // [T][2n-3] unrooted, [T][2n-2] rooted
  const double* bl;           // [T][2n-2] unrooted, [T][2n-1] rooted
  const double* rates;        // [T][2n-2] or nullptr: branch length x rate
  int32_t* scratch;           // [T][13 N]
  SchedEntry* sched;          // [T][n-1]
  MacroEntry* macros;         // [T][max_macros(n)] (may be nullptr)
  int32_t* macro_count;       // [T]
  double* bl_eff;             // [T][N]
  int32_t* status;            // [2]: code, tree
  int max_slots;
  int use_lds;     // set by the launcher
  int need_slots;  // 0: no log-likelihood kernel will run on this batch (node-id order, no LDS slots)
  // arena calls: the slot assignment of launch_macro_slots done by the tree's set-up workgroup
  // (tree_setup_wg_kernel only; launch_setup says whether it was): outputs, or nullptr
  MacroEntry* arena_macros;  // [T][max_macros(n)]
  int32_t* slot_need;        // [T]
  int arena_sure;            // set by the launcher
};

struct ModelSetupArgs {
  int T, models_per_tree;
  int subst, site, K;
  int param_count, rates_off, freqs_off, shape_off;
  const double* params;  // [T][param_count]
  DevModel* models;      // [T * models_per_tree]
  int32_t* status;
  const double* weibull_x;  // [K][2]: {x_k, log x_k} of the Weibull quantiles (launch_weibull_table), or nullptr
};

struct TransitionArgs {
  int E, N, K;
  EvalMap map;
  const DevModel* models;
  const double* bl_eff;  // [T][N]
  double* mats;          // [E][N-1][K][16]
  double* tip_tables;    // [E][n][K][5][4]: per tip edge and state (4 = gap), the column of P; may be nullptr
  int n;
  int ev_skip_begin, ev_skip_end;  // evaluations [begin, end) are not walked at all: no matrices
  int eval_base;                   // this launch covers evaluations [eval_base, eval_base + E)
};

// Matrices in the order the second-generation gradient walk consumes them (kernels_walk.hip):
// gradient evaluations [eval_begin, eval_begin + count) of the call, written to
// mmats[0 .. count) (the caller passes the pointer of the first one).
struct TransitionMacroArgs {
  int n, N, K, count, eval_begin;
  EvalMap map;
  const DevModel* models;
  const double* bl_eff;        // [T][N]
  const MacroEntry* macros;    // [T][max_macros(n)] (the order the walk uses)
  const int32_t* macro_count;  // [T]
  double* mmats;               // [count][max_macros(n)][6][K][16]{f, tr}
  double* mphi;                // [count][max_macros(n)][6][K][16] or nullptr
};

struct LikArgs {
  int n, N, P, K, tiles;
  int lds_slots;    // PLV slots in LDS (set by the launcher)
  // second-generation gradient walk (set by its launcher): the launch's evaluations, how many
  // of them (the first ones) are walked by `walk_groups` waves that take several pattern
  // tiles each (tile g, g + walk_groups, ...); the others get a wave per tile
  int walk_evals, walk_big_evals, walk_groups;
  int store;           // matrix-core gradient kernels: 0 = the launcher decides, 1 = stored vectors in LDS, 2 = arena (the engine decides: its schedules must match)
  const uint8_t* tip_code_tiles;  // look-up walk: tip_codes by pattern tile in the form its LDS holds them (launch_tip_code_tiles), or nullptr
  const uint8_t* tip_tiles;  // loglik_mfma_kernel: tip_masks by pattern tile in the kernel's LDS layout, or nullptr
  int tile_regs;       // look-up walk: registers per vector = tile width (0: the default, kLlR; 4: wide tiles -- gradient_walk_tile_regs)
  int evals_per_wave;  // loglik_mfma_kernel: consecutive evaluations of one tree per wave (launcher)
  int kp;           // MFMA path: categories per instruction (1, 2 or 4; set by the launcher)
  int cat_groups;   // matrix-core gradient: groups of four categories (K > 4; set by the launcher)
  int ll_tiles;     // stride of ll_part per evaluation (>= partial sums any kernel writes)
  int g_tiles;      // stride of g_part per gradient evaluation = tiles of the gradient kernel used
  int eval_offset;  // first evaluation of this launch
  int grad_offset;  // gradient-workspace index of that evaluation
  EvalMap map;
  const DevModel* models;
  const SchedEntry* sched;
  const MacroEntry* macros;    // [T][max_macros(n)]
  const int32_t* macro_count;  // [T]
  const double* mats;
  const double* tip_tables;    // see TransitionArgs
  const double* mmats;         // see TransitionMacroArgs (indexed by gradient evaluation)
  const double* mphi;
  const int8_t* tip_states;    // [n][P]
  const uint8_t* tip_masks;    // [n][P] bit s: compatible with state s (matrix-core gradient)
  const uint8_t* tip_codes;    // [n][P] 16 x state, 64 = gap (third-generation walk: byte offset of the state's table entry)
  const double* tip_partials;  // [n][P][4] or nullptr
  const double* weights;       // [P]
  double* ll_part;             // [E][tiles]
  double* plv;                 // [Eg][n-1][K][tiles*64][4]   (gradient, v1)
  double* g_part;              // [Eg][tiles][2][N]
  double* site_lik;            // [Eg][tiles*64] per-pattern site likelihood (K > 4 gradient: from the logL pass)
  int32_t* site_exp;           // [Eg][tiles*64] its power of two when rescaling
  int32_t* status;             // [4]: code, tree (schedule does not fit the kernel's LDS slots), [2]: 1 + tree of a walk wave of the one-launch call that waited in vain
  const int32_t* slot_need;    // [T] arena gradient kernel: LDS slots each tree's schedule uses
  int lds_lo;                  // arena gradient kernel: this launch takes trees with lds_lo < need <= lds_slots
  double* pattern_ll;          // [T][P] log-likelihood kernels' PATTERN_LL variant: unweighted log L_p per (tree, pattern); else nullptr
  const uint8_t* pattern_blank;  // [P] PATTERN_LL variant: 1 where every tip vector of the pattern is all ones (L_p = 1 exactly: reported as 0.0)
  // ancestral_hbm_kernel (kernels_ancestral.hip) only, by the call's tree index; nullptr in every
  // other call, and there each but anc_state may be nullptr (no work, no stores)
  double* anc_state;  // [T][n-2][P][4] state posteriors of the internal nodes n .. 2n-3
  int8_t* anc_map;    // [T][n-2][P] their largest entry
  double* anc_cat;    // [T][P][K] rate-category posteriors
  double* anc_rate;   // [T][P] posterior mean rate
  double* anc_tip;    // [T][n][P][4] state posteriors at the leaves
  // placement_table_hbm_kernel (kernels_placement.hip) only; nullptr / 0 in every other call
  const double* place_half;  // [T][N-1][K][16] P(r_k t_e / 2) by node id, as `mats`
  const double* place_pend;  // [T][G][K][16] P(r_k l_g) of the pendant lengths
  double* place_table;       // [trees of the table launch][2n-3][G][5][tiles*64]: S of DESIGN.md 4.17
  int place_G;               // pendant lengths, 1 .. kPlacementMaxPendants
  int place_tree0;           // the call's tree that row 0 of place_table belongs to
};

// How many logL partial sums each evaluation's walk kernel wrote (the kernels tile the
// patterns differently): `mid` for evaluations [mid_lo, mid_hi) -- the finite-difference
// passes of a GTR gradient call --, `ends` for the others.  Consumers sum exactly those.
struct LlCounts {
  int ends, mid, mid_lo, mid_hi;
  __host__ __device__ int of(long e) const { return (e >= mid_lo && e < mid_hi) ? mid : ends; }
};

struct FinalizeArgs {
  int n, N, T, K, tiles;
  int ll_tiles;  // stride of ll_part per evaluation
  LlCounts ll_used;
  int g_tiles;   // gradient partial sums per gradient evaluation
  int gradient, rooted, with_jacobian;
  int gtr, site_fused, site_separate;
  const double* ll_part;
  const double* g_part;
  const double* bl_eff;        // [T][N]
  const double* bl_raw;        // rooted: [T][N]
  const double* rates;         // rooted: [T][N-1]
  const int32_t* rate_counts;  // rooted gradient: [T]
  const double* node_heights;  // [T][N]
  const double* node_bounds;   // [T][N]
  const double* height_ratios; // [T][n-1]
  const SchedEntry* sched;     // [T][n-1]
  double* scratch;             // [T][6 n]
  double* out_ll;              // [T]
  double* out_branch;          // unrooted gradient: [T][N]
  double* out_ratios;          // rooted gradient: [T][n-1]
  double* out_clock;           // rooted gradient: [T][N-1]
  double* out_site;            // [T] or nullptr
  double* out_subst;           // [T][8] or nullptr
  int32_t* status;
  int use_lds;  // set by the launcher
  int32_t* clear_ready;  // reduce_finalize: the one-launch call's hand-off words, zeroed per tree (or nullptr)
};

// tree schedules (one wave per tree) and model instances (one thread each) in one launch
// (returns true when the arena's slot assignment was done in the same launch: a.arena_macros)
// (sw: MI_PHYLO_TREE_SETUP, MI_PHYLO_MACRO_SLOTS)
bool launch_setup(const TreeSetupArgs& a, const ModelSetupArgs& ms, const Switches& sw, hipStream_t s);
bool launch_tree_setup(const TreeSetupArgs& a, const Switches& sw, hipStream_t s);  // (as launch_setup)  // trees only
void launch_weibull_table(int K, double* table, hipStream_t s);  // once per engine: ModelSetupArgs::weibull_x
void launch_transition(const TransitionArgs& a, hipStream_t s);
// On-chip (LDS-resident) log-likelihood: evaluations [eval_offset, eval_offset+count)
// (sw: MI_PHYLO_LOGLIK_PATH, MI_PHYLO_LOGLIK_EVALS_PER_WAVE)
void launch_loglik(const LikArgs& a, int count, bool rescale, int max_slots, const Switches& sw, hipStream_t s);
int loglik_mfma_tiles(int P, int K);
// the matrix-core log-likelihood kernel's tip bytes, pre-tiled once per engine (LikArgs::tip_tiles)
size_t loglik_tip_tiles_bytes(int n, int P, int K);
void launch_tip_tiles(const uint8_t* masks, uint8_t* tiles, int n, int P, int K, hipStream_t s);
int gradient_mfma_tiles(int P, int K, int regs = 0);  // regs: registers per vector (0: kLlR)
// the look-up walk's tip codes pre-tiled once per engine for its tile width (LikArgs::tip_code_tiles)
size_t tip_code_tiles_bytes(int n, int P, int K, int regs);
void launch_tip_code_tiles(const uint8_t* codes, uint8_t* out, int n, int P, int K, int regs, hipStream_t s);
// tile width of the look-up walk for an engine whose batches take the arena (kLlR or 4:
// kernels_walk3.hip, RR; forced: MI_PHYLO_WALK_TILE_REGS, 0 if unset)
int gradient_walk_tile_regs(int n, int P, int K, int forced);
// Gradient, partial-likelihood vectors streamed through HBM (any tree size, rescaling)
void launch_gradient_hbm(const LikArgs& a, int count, bool rescale, hipStream_t s);
// ... its branch-length Hessian form (one evaluation per tree; g_part [Eg][tiles][3][N]:
// sums of w D1/L, w D2/L and w (D1/L)^2 by node id -- DESIGN.md 4.8)
void launch_gradient_hbm_hessian(const LikArgs& a, int count, bool rescale, hipStream_t s);
const char* gradient_hessian_kernel_name();
// ... and the Hessian form of the second-generation walk (kernels_walk.hip; K <= 4, tip masks):
// g_part [Eg][tiles][Mmax][6][2] = {sum w D1/L, sum w D2/L} by (macro, position), then
// [Mmax][6] sums of w (D1/L)^2; a wave per pattern tile; a.store: 1 LDS, 2 arena
void launch_gradient_walk_hessian(const LikArgs& a, int count, bool rescale, hipStream_t s);
const char* gradient_walk_hess_kernel_name();
// The Hessian call's tile reduction and finalize, a workgroup per tree (kernels_finalize.hip)
struct HessFinalizeArgs {
  int N, T, g_tiles, ll_tiles, ll_used;
  // walk form (positional sums; macros == nullptr: the HBM kernel's [3][N] by node id)
  int n, g_width;
  const MacroEntry* macros;    // [T][macro_stride(n)], the order the walk used
  const int32_t* macro_count;  // [T]
  const double* ll_part;  // [T][ll_tiles]
  const double* g_part;   // [T][g_tiles][3][N]
  double* out_ll;         // [T] or nullptr
  double* out_branch;     // [T][N] or nullptr
  double* out_hess;       // [T][N]: sum w D2/L - sum w (D1/L)^2
  double* out_gsq;        // [T][N] or nullptr: sum w (D1/L)^2
};
void launch_hessian_finalize(const HessFinalizeArgs& a, hipStream_t s);
// The NNI neighbourhood scan (kernels_nni.hip): the HBM-streamed walk with, per
// inner edge, the log-likelihood change of its two interchanges; one evaluation per tree;
// g_part [Eg][tiles][2][N] by node id.  Its tile reduction and outputs, a workgroup per tree.
void launch_nni_scan_hbm(const LikArgs& a, int count, bool rescale, hipStream_t s);
const char* nni_scan_kernel_name();
struct NniFinalizeArgs {
  int N, n, T, g_tiles, ll_tiles, ll_used;
  const double* ll_part;  // [T][ll_tiles]
  const double* g_part;   // [T][g_tiles][2][N]
  double* out_ll;         // [T] or nullptr
  double* out_delta;      // [T][N][2]
  int32_t* out_best;      // [T] or nullptr: 2 v + i of the largest delta (-1: no inner edge)
};
void launch_nni_finalize(const NniFinalizeArgs& a, hipStream_t s);
// Marginal ancestral-state and rate-category posteriors (kernels_ancestral.hip):
// the HBM-streamed walk with, per internal node and pattern, the normalised joint of the node's
// state and the data (LikArgs::anc_*); one evaluation per tree.  Its log-likelihoods from the
// tile partials [T][ll_tiles], the first ll_used of each, in the scan's order (out_ll == nullptr:
// no launch).
void launch_ancestral_hbm(const LikArgs& a, int count, bool rescale, hipStream_t s);
void launch_ancestral_finalize(const double* ll_part, int T, int ll_tiles, int ll_used, double* out_ll,
                               hipStream_t s);
const char* ancestral_kernel_name();
// Phylogenetic placement (kernels_placement.hip): the HBM-streamed walk with, per
// caller edge, pendant length and pattern, the five log-likelihoods of "the query shows A / C / G /
// T / gap" at the edge's midpoint (LikArgs::place_*); the gather-and-sum of the queries over that
// table; best edge and likelihood weight ratios per (tree, query).
constexpr int kPlacementMaxPendants = 4;  // MI_PLACEMENT_MAX_PENDANTS
constexpr int kPlacementQueryBlock = 128;  // queries a scoring workgroup streams through its edge's table
void launch_placement_table_hbm(const LikArgs& a, int count, bool rescale, hipStream_t s);
const char* placement_kernel_name();
// halved effective lengths [T][N], the pendant lengths as rows [T][G+1] (what launch_transition
// reads), and the checks a device-pointer call cannot make on the host (status word)
struct PlacePrepareArgs {
  int T, N, G, C, P;
  const double* bl_eff;           // [T][N]
  const double* pendant_lengths;  // [G]
  const int32_t* column_pattern;  // [C]
  double* half_bl;                // [T][N]
  double* pend_bl;                // [T][G+1]
  int32_t* status;
};
void launch_placement_prepare(const PlacePrepareArgs& a, hipStream_t s);
struct PlaceScoreArgs {
  int trees, tree0;  // trees of `table`, the call's tree of its row 0
  int E, G, P, Q, C;
  size_t ppad;       // patterns of a table row (tiles * 64)
  int use_lds;       // 1: a workgroup copies its edge's [G][5][ppad] into LDS; 0: it gathers from `table`
  const double* table;            // [trees][E][G][5][ppad]
  const int8_t* query_states;     // [Q][C]
  const int32_t* column_pattern;  // [C]
  const double* column_weights;   // [C] or nullptr: 1
  double* edge_ll;                // [T][Q][E] by the call's tree
  int8_t* pendant_index;          // [T][Q][E] or nullptr
};
bool placement_table_fits_lds(int G, size_t ppad);
void launch_placement_score(const PlaceScoreArgs& a, hipStream_t s);
// S itself for the caller: [trees][E][G][5][ppad] -> out [T][E][G][5][P] by the call's tree
void launch_placement_table_copy(const double* table, int trees, int tree0, int E, int G, int P, size_t ppad,
                                 double* out, hipStream_t s);
struct PlaceFinalizeArgs {
  int T, Q, E, ll_tiles, ll_used;
  const double* ll_part;   // [T][ll_tiles]
  const double* edge_ll;   // [T][Q][E]
  double* out_ll;          // [T] or nullptr
  int32_t* out_best_edge;  // [T][Q] or nullptr
  double* out_lwr;         // [T][Q][E] or nullptr
};
void launch_placement_finalize(const PlaceFinalizeArgs& a, hipStream_t s);
// The SPR neighbourhood scan (kernels_spr.hip): the HBM-streamed walk that keeps
// the vectors of both directions at every edge with their cumulative rescaling exponents
// (spr_vectors_hbm_kernel: LikArgs as every member, SprArgs beside it), the regraft walk over
// every (tree, tile, pruned edge), and the tile sums with the best target per (s, dir) and the best
// move per tree.  One SprArgs describes a launch of `trees` trees; the workspaces are indexed by
// the tree of the launch, the outputs by the call's tree (tree0 + ...).  E = 2n-3.
struct SprArgs {
  int n, K, P, tiles;
  int trees, tree0;
  int radius;       // 0: every move; else moves of distance <= radius
  int depth_slots;  // messages of a regraft wave's path
  int waves;        // regraft waves of a launch: each owns a path workspace and takes job after job
  int ll_tiles, ll_used;
  const DevModel* models;       // [T]
  const SchedEntry* sched;      // [T][n-1]
  const double* mats;           // [T][2n-2][K][16] by node id
  const double* half;           // [T][2n-2][K][16] P(r_k t_e / 2) by node id
  const double* weights;        // [P]
  const int8_t* tip_states;     // [n][P]
  const double* tip_partials;   // [n][P][4] or nullptr
  const double* down;           // LikArgs::plv: [trees][n-1][K][tiles*64][4] post-order vectors
  double* up;                   // [trees][2n-2][K][tiles*64][4] vectors at the top of every edge
  int32_t* exp_down;            // [trees][n-1][tiles*64] cumulative exponents of `down` (rescaling)
  int32_t* exp_up;              // [trees][2n-2][tiles*64] ... of `up`
  double* site;                 // [trees][tiles*64] L_p = site 2^site_exp
  int32_t* site_exp;            // [trees][tiles*64]
  double* path;                 // [waves][depth_slots + 1][K][64][4] messages of the current path, the moving part
  int32_t* path_exp;            // [waves][depth_slots][64] their exponents (rescaling)
  double* part;                 // [trees][tiles][2E][E] per-tile partial sums of w_p log(L'_p / L_p)
  const double* ll_part;        // [T][ll_tiles]
  double* out_ll;               // [T] or nullptr
  int32_t* out_best_target;     // [T][E][2]
  double* out_best_delta;       // [T][E][2]
  int32_t* out_best_move;       // [T][3] or nullptr
  double* out_delta;            // [T][E][2][E] or nullptr
};
void launch_spr_half_lengths(const double* bl_eff, size_t count, double* half_bl, hipStream_t s);
void launch_spr_vectors_hbm(const LikArgs& a, const SprArgs& w, int count, bool rescale, hipStream_t s);
const char* spr_kernel_name();
bool spr_regraft_fits_lds(int n, int depth_slots);  // the tree and the walk's frames in 64 KiB
void launch_spr_regraft(const SprArgs& a, bool rescale, hipStream_t s);
void launch_spr_finalize(const SprArgs& a, hipStream_t s);
// Branch-length optimisation (kernels_branch_opt.hip): the step between two
// Hessian passes and the packing of the active trees.  "Packed" arrays hold the trees that
// are still being evaluated, in `map` order (map == nullptr: all trees, in their own order).
constexpr int kBranchOptActive = -1;  // internal; the rest are mi_phylo.h's MI_BRANCH_OPT_*
constexpr int kBranchOptConverged = 0, kBranchOptIterationLimit = 1, kBranchOptStalled = 2;
struct BranchOptArgs {
  int N, T;        // nodes per tree (2n-1), trees of the batch
  int count;       // trees of the packed set
  int evals_max;   // evaluations a tree may use
  int pass;        // index of this pass: its word of `active`
  double tol, tmin, tmax;
  const int32_t* map;  // [count] packed position -> tree, or nullptr
  // what the Hessian pass returned for the trial points, by packed position
  const double *tr_ll, *tr_g, *tr_h, *tr_s;  // [count], [count][N] each
  double* trial;       // [count][N-1] trial lengths: evaluated ones in, next ones out
  double* trial_full;  // [T][N-1] the same by tree (what a later packing reads), or nullptr
  // the accepted point, by tree: these are the call's outputs
  double *bl, *ll, *g, *h, *s, *alpha;  // [T][N-1], [T], [T][N] x 3, [T]
  int32_t *evals, *status;              // [T]
  int32_t* active;  // [passes] trees still active after each pass (zeroed by the host)
};
struct BranchOptPackArgs {
  int N, count, param_count;  // count: trees of the NEW packed set
  int32_t* map;               // [count] new map (written by the scan, read by the gather)
  const int32_t* parent_ids;  // [T][N-2] the caller's
  const double* params;       // [T][param_count] the caller's
  const double* trial_full;   // [T][N-1]
  int32_t* pk_parent;         // [count][N-2]
  double* pk_trial;           // [count][N-1]
  double* pk_params;          // [count][param_count]
};
void launch_branch_opt_init(const BranchOptArgs& a, const double* start, hipStream_t s);
void launch_branch_opt_step(const BranchOptArgs& a, hipStream_t s);
void launch_branch_opt_pack(const BranchOptPackArgs& a, int old_count, const int32_t* map_old,
                            const int32_t* status, hipStream_t s);
// The hill-climbing searches (kernels_search.hip): taking NNI and SPR
// moves on the device in the reference's numbering, and the per-tree step between two rounds of
// a search.  A wave per tree; the working arrays of a tree (NNI: six of 2n-2 words and eight
// more, SPR: seven) are in LDS up to k{Nni,Spr}ApplyLdsNodes nodes, else in `ws`.
constexpr int kNniApplyLdsNodes = 512, kNniApplyArrays = 6, kNniApplyExtra = 8;
constexpr int kSprApplyLdsNodes = 512, kSprApplyArrays = 7, kSprApplyExtra = 8;
inline __host__ __device__ size_t nni_apply_ws_words(int n) {  // per tree; 0: the arrays are in LDS
  const size_t R = 2 * (size_t)n - 2;
  return R > kNniApplyLdsNodes ? kNniApplyArrays * R + kNniApplyExtra : 0;
}
inline __host__ __device__ size_t spr_apply_ws_words(int n) {
  const size_t R = 2 * (size_t)n - 2;
  return R > kSprApplyLdsNodes ? kSprApplyArrays * R + kSprApplyExtra : 0;
}
struct MoveApplyArgs {
  int n, T;
  const int32_t* parent_ids;  // [T][2n-3]
  const double* bl;           // [T][2n-2]
  const int32_t* moves;       // NNI [T]: 2 v + i, or -1: copy; SPR [T][3]: (s, dir, f), or (-1, -1, -1): copy
  int32_t* ws;                // [T][{nni,spr}_apply_ws_words(n)]
  int32_t* status;            // the engine's status word
  int32_t* out_parent_ids;    // [T][2n-3]  (no output may overlap an input)
  double* out_bl;             // [T][2n-2]
};
void launch_nni_apply(const MoveApplyArgs& a, hipStream_t s);
void launch_spr_apply(const MoveApplyArgs& a, hipStream_t s);
constexpr int kSearchActive = -1;  // internal; the rest are mi_phylo.h's MI_{NNI,SPR}_SEARCH_*
struct SearchStepArgs {
  int n, count, round, max_moves;  // count: trees of the packed set
  double min_gain;
  const int32_t* map;  // [count] packed position -> tree, or nullptr
  // this round's results, by packed position
  const double *opt_bl, *opt_ll;  // [count][2n-2], [count]
  const int32_t* opt_status;      // [count]
  const double* delta;            // NNI [count][2n-1][2]; SPR [count][2n-3][2], the scan's best_delta
  const int32_t* best;            // NNI [count]; SPR [count][3], the scan's best_move
  // the trees by tree index: this round's and the other half of the pair
  const int32_t* cur_pid;  // [T][2n-3]
  double* cur_bl;          // [T][2n-2]
  int32_t* next_pid;
  double* next_bl;
  // the packed inputs of the next round (map != nullptr)
  int32_t* pk_pid;  // [count][2n-3]
  double* pk_bl;    // [count][2n-2]
  int32_t* ws;      // [count][{nni,spr}_apply_ws_words(n)]
  int32_t* engine_status;
  // the call's outputs, by tree
  int32_t* out_pid;
  double *out_bl, *out_ll, *out_best_delta;  // (out_best_delta may be nullptr)
  int32_t *move_count, *move_log;            // [T], NNI [T][max_moves] / SPR [T][max_moves][3] or nullptr
  double* move_gain;                         // [T][max_moves] or nullptr
  int32_t *status, *out_opt_status;          // [T] kSearchActive while searching; [T] or nullptr
  int32_t* active;                           // this round's word: trees that moved
};
void launch_nni_search_step(const SearchStepArgs& a, hipStream_t s);
void launch_spr_search_step(const SearchStepArgs& a, hipStream_t s);
// RELL re-summation and the tree-mixture marginal (kernels_rell.hip)
struct RellArgs {
  int B, T, P;
  const double* pattern_ll;  // [T][P]
  const double* weights;     // [B][P]
  double* c;                 // [B][T] the product (the caller's or the engine's)
  double* row_max;           // [B] row maxima m_b
  double* row_inv;           // [B] 1 / sum_t exp(C[b][t] - m_b)
  int32_t* counts;           // [T] replicates won (zeroed before the launch)
  int32_t* best;             // [B] or nullptr
  double* bp;                // [T]
  double* elw;               // [T] or nullptr
};
void launch_rell(const RellArgs& a, hipStream_t s);  // product, row pass, column pass
// once per 4-state engine: blank[p] = 1 where every tip vector of pattern p is all ones (an all-gap
// column), from the state masks [n][P] or, without them, the partials [n][P][4]
void launch_pattern_blank(const uint8_t* masks, const double* partials, int n, int P, uint8_t* blank, hipStream_t s);
const char* rell_product_kernel_name();
struct MixtureArgs {
  int T, P;
  const double* pattern_ll;       // [T][P]
  const double* log_weights;      // [T] or nullptr: log(1/T) each
  const double* pattern_weights;  // [P]
  double* out_pattern;            // [P]
  double* out_total;              // [1]
};
void launch_pattern_mixture(const MixtureArgs& a, hipStream_t s);
// kernels_boot.hip: multiscale bootstrap weights drawn on the device and the KH, SH and AU tests on
// the RELL matrices.  The sampler: a workgroup per replicate (grid-stride), its
// draws dealt over the lanes, an int32 histogram of the replicate's P counts in LDS -- with the
// prefix sum beside it, (2 P + 1) words -- up to kBootLdsPatterns patterns, else in a row of `hist`.
constexpr int kBootThreads = 256;
constexpr int kBootLdsPatterns = 6144;  // (2 P + 1) words <= 48 KiB + 4: three workgroups share a CU's 160 KiB
constexpr int kBootLdsGrid = 2048;      // workgroups of the LDS form, at most
constexpr int kBootGlobalRows = 1024;   // workgroups of the global form = histogram rows of the workspace, at most
inline bool boot_hist_global(int P, bool forced) { return forced || P > kBootLdsPatterns; }
inline int boot_hist_rows(int B, int P, bool forced) {  // rows of BootArgs::hist
  return boot_hist_global(P, forced) ? (B < kBootGlobalRows ? B : kBootGlobalRows) : 0;
}
struct BootArgs {
  int P, B;
  int global_hist;           // 1: the histograms are rows of `hist` (boot_hist_global)
  uint64_t sites;            // n: draws per replicate
  uint64_t seed;
  uint64_t first_replicate;  // replicate b of the launch is number first_replicate + b
  int64_t expect_total;      // the prefix sum: N must equal it (kBootSitesNotTotal), or -1
  const double* weights;     // [P] the prefix sum's input
  uint32_t* cum;             // [P + 1] exclusive prefix sum of the weights, cum[P] = N
  uint32_t* total;           // [1] N; 0 where the weights were refused: the sampler then writes zeros
  int32_t* hist;             // [boot_hist_rows][P] or nullptr
  int32_t* status;           // the engine's status word
  double* out;               // [B][P]
};
void launch_boot_prefix(const BootArgs& a, hipStream_t s);  // checks, cum, total
void launch_boot_sample(const BootArgs& a, hipStream_t s);
void launch_boot_zero(int32_t* words, size_t count, hipStream_t s);  // a call's integer counters
// The tests: what is made of block 0's product C [B][T] (column means, row maxima of the centred
// matrix, the KH and SH counts), and the table from those, the observed log-likelihoods and every
// block's counts.  The blocks' sizes travel by value: a captured call keeps no host pointer.
constexpr int kTopoMaxScales = 64;  // MI_TOPOLOGY_MAX_SCALES
constexpr int kTopoColumns = 11;    // MI_TOPOLOGY_COLUMNS
struct TopoArgs {
  int T, B, K;            // trees, replicates of block 0, blocks
  const double* c;        // [B][T] block 0's product
  const double* L;        // [T] observed log-likelihoods
  const int32_t* counts;  // [K][T] replicates won per block
  const double* bp;       // [T] block 0's bootstrap proportions
  const double* elw;      // [T] ... and expected-likelihood weights
  const uint32_t* total;  // [1] N
  double* mean;           // [T]
  double* zmax;           // [B] workspace: max_t (C[b][t] - mean[t])
  int32_t* sel;           // [2] workspace: t1, t2 (-1: T = 1)
  int32_t* sh;            // [T] workspace, zeroed: SH counts
  int32_t* kh;            // [T] workspace, zeroed: KH counts
  double* table;          // [T][kTopoColumns]
  int64_t sites[kTopoMaxScales];
  int32_t replicates[kTopoMaxScales];
};
void launch_topo_block0(const TopoArgs& a, hipStream_t s);  // best two, means, row maxima, counts
void launch_topo_table(const TopoArgs& a, hipStream_t s);
// Starting trees.  kernels_distance.hip: the substitution counts of all pairs of
// taxa for B sets of pattern weights on the matrix cores, and each pair's maximum-likelihood
// distance.  The tip codes [distance_code_rows(n)][distance_code_stride(P)] (a byte each: the
// state, 4 = missing, the padding included) are made once per engine.
inline __host__ __device__ int distance_code_rows(int n) { return (n + 3) & ~3; }
inline __host__ __device__ int distance_code_stride(int P) { return (P + 15) & ~15; }
void launch_distance_codes(const int8_t* states, const double* partials /* or nullptr: the states */, int n, int P,
                           uint8_t* codes, hipStream_t s);
struct DistanceArgs {
  int n, n4, P, Pp, K;
  int B;                  // replicates of this launch (a chunk of the call's)
  const uint8_t* codes;   // [n4][Pp]
  const double* weights;  // [B][P]
  double* counts;         // [B][n(n-1)/2][16] workspace
  const DevModel* model;  // the call's one model instance
  double tmin, tmax, tol;
  int max_iter;
  double* out_dist;      // [B][n][n]
  double* out_counts;    // [B][n(n-1)/2][16] or nullptr
  int8_t* out_status;    // [B][n(n-1)/2] or nullptr
};
void launch_pair_distances(const DistanceArgs& a, hipStream_t s);  // counts, then distances
const char* pair_counts_kernel_name();
// kernels_nj.hip: neighbour joining of B distance matrices, a wave per matrix, the tree written in
// the reference's numbering.  The working set of a matrix (nj_ws_bytes) is in LDS up to
// kNjLdsTaxa taxa, else in `ws`.
constexpr int kNjLdsTaxa = 128;
inline __host__ __device__ size_t nj_ws_bytes(int n) {  // per matrix, a multiple of 256
  const size_t R = 2 * (size_t)n - 2;
  const size_t doubles = (size_t)n * n + n + R, words = n + R + kNniApplyArrays * R + kNniApplyExtra;
  return (8 * doubles + 4 * words + 255) & ~(size_t)255;
}
struct NjArgs {
  int n, B;
  double tmin, tmax;
  const double* dist;        // [B][n][n], i < j read
  char* ws;                  // [B][nj_ws_bytes(n)] (n > kNjLdsTaxa)
  int32_t* status;           // the engine's status word
  int32_t* out_parent_ids;   // [B][2n-3]
  double* out_bl;            // [B][2n-2]
};
// the large-LDS opt-in of the kernel for n taxa: launch_nj makes it on a first launch of that
// size, which must not happen inside a graph capture -- a reservation calls this beforehand
void nj_prepare(int n);
void launch_nj(const NjArgs& a, hipStream_t s);
// kernels_splits.hip: the split table of a batch of unrooted trees and the Robinson-Foulds
// distances from its indices.  An occurrence is an edge of a tree, numbered
// o = t (2n-3) + v.  A wave of tree_splits_kernel owns 64 / split_lane_words(n) trees; a tree's
// working bitsets ([2n-2 nodes][64 lanes] words per wave) are in LDS up to kSplitLdsTaxa taxa,
// else in `store`.
constexpr int kSplitLdsTaxa = 128;
constexpr int kRfMaxTaxa = 2049;  // (a tree's sorted list, padded to a power of two, in 48 KiB of LDS)
inline __host__ __device__ int split_words(int n) { return (n + 31) >> 5; }
// words a tree's lanes take at once: the power of two at or above split_words(n), 64 at most
inline __host__ __device__ int split_lane_words(int n) {
  int w = 1;
  while (w < split_words(n) && w < 64) w <<= 1;
  return w;
}
inline __host__ __device__ size_t split_store_bytes_per_wave(int n) { return (2 * (size_t)n - 2) * 64 * 4; }
inline size_t split_wave_count(int T, int n) {
  const int per = 64 / split_lane_words(n);
  return ((size_t)T + per - 1) / per;
}
inline size_t split_table_slots(size_t occurrences) {  // a power of two >= 2 x occurrences
  size_t h = 2;
  while (h < 2 * occurrences) h <<= 1;
  return h;
}
struct SplitArgs {
  int n, T, W, capacity;
  int hash_bits;              // the hash is masked to that many bits before the first probe (32: all)
  uint32_t slots;             // table slots, a power of two
  const int32_t* parent_ids;  // [T][2n-3]
  const double* bl;           // [T][2n-2] or nullptr
  const double* weights;      // [T] or nullptr
  int32_t* status;            // the engine's status word
  // workspace
  uint32_t* store;      // [waves][2n-2][64] working bitsets (n > kSplitLdsTaxa)
  uint32_t* occ_bits;   // [O][W] the canonical split of every occurrence
  uint64_t* occ_hash;   // [O]; after the insertion: uint32 flags [O] | uint32 ranks [O]
  int32_t* occ_slot;    // [O] the table slot of the occurrence's split (between the word passes
                        // of tree_splits_kernel: 1 where the leaf set held taxon 0)
  void* scan_tmp;       // rocPRIM's temporary storage of the scan
  size_t scan_tmp_bytes;
  int32_t* slot_owner;  // [slots] -1, or the occurrence that claimed the slot
  int32_t* slot_first;  // [slots] the lowest occurrence number of the slot's split
  int32_t* slot_trees;  // [slots] occurrences of the slot's split
  // the statistics' sort (out_stats only): keys = split index, values = occurrence
  uint32_t *keys, *vals, *keys2, *vals2;
  void* sort_tmp;
  size_t sort_tmp_bytes;
  // outputs
  int32_t* out_index;   // [T][2n-1]
  int32_t* out_count;   // [1]
  uint32_t* out_bits;   // [capacity][W]
  int32_t* out_first;   // [capacity]
  int32_t* out_trees;   // [capacity]
  double* out_stats;    // [capacity][3] or nullptr
};
size_t split_scan_tmp_bytes(size_t occurrences);
size_t split_sort_tmp_bytes(size_t occurrences);
int launch_split_index(const SplitArgs& a, hipStream_t s);  // nonzero: rocPRIM refused a launch
struct RfArgs {
  int n, T;
  const int32_t* split_index;  // [T][2n-1]
  const double* bl;            // [T][2n-2] or nullptr
  int32_t* sorted_index;       // [T][2n-3] workspace: a tree's nonnegative indices, ascending
  double* sorted_length;       // [T][2n-3] workspace: their lengths
  int32_t* sorted_count;       // [T] workspace
  int32_t* out_rf;             // [T][T]
  double* out_bs;              // [T][T] or nullptr
};
void launch_rf(const RfArgs& a, hipStream_t s);
// kernels_sbn.hip: subsplit Bayesian networks over tree batches.  A tree has
// E = 2n-3 edges, 2E directed edges d = 2v + s and 3 slots per directed edge; a PCSP occurrence
// is numbered o = (t 2E + d) 3 + k.  The per-tree kernels give a tree to a LANE; a wave holds
// `tpw` trees (MI_PHYLO_SBN_TREES_PER_WAVE) and the per-node arrays of its trees, six 32-bit
// words per node laid out [word][node][tpw], are in LDS while they fit 160 KiB, else in `store`.
constexpr int kSbnNodeWords = 6;  // child 0, child 1, two doubles (or four ints)
constexpr int kSbnDefaultTreesPerWave = 16;
inline __host__ __device__ size_t sbn_store_bytes_per_wave(int n, int tpw) {
  return (2 * (size_t)n - 2) * kSbnNodeWords * 4 * tpw;
}
inline int sbn_lds_taxa(int tpw) { return (int)((160 * 1024 / (kSbnNodeWords * 4 * tpw) + 2) / 2); }
inline size_t sbn_wave_count(int T, int tpw) { return ((size_t)T + tpw - 1) / tpw; }
struct SbnIndexArgs {
  int n, T, T0, W, tpw;
  int root_capacity, pcsp_capacity;
  int hash_bits;
  uint32_t slots;               // table slots (each of the two tables), a power of two
  const int32_t* parent_ids;    // [T][2n-3]
  int32_t* status;
  // workspace
  char* store;                  // [waves][sbn_store_bytes_per_wave] (n > sbn_lds_taxa)
  const int32_t* split_index;   // [T][2n-1] of the whole batch
  const int32_t* split_first;   // [T (2n-3)] first occurrences of the batch's splits
  const int32_t* split_count;   // [1]
  const uint32_t* split_bits;   // [T (2n-3)][W]
  int32_t* counts;              // [4] S, C, parents, spare
  int32_t* occ_key;             // [O][3] sister, focal, child clades (2 split + side); sister -1: no such slot
  int32_t* occ_slot;            // [O] slot in the PCSP table
  int32_t* occ_pslot;           // [O] slot in the parent table
  int32_t *slot_owner, *slot_first, *pslot_owner, *pslot_first;  // [slots] each
  uint64_t *keys, *keys2;       // [O] (parent's first occurrence, own first occurrence); all ones: not a first occurrence
  uint32_t *vals, *vals2;       // [O]
  uint32_t *heads, *head_scan;  // [O] block heads in sorted order and their inclusive scan
  int32_t* rank_of;             // [O] sorted position of a first occurrence
  void *sort_tmp, *scan_tmp;
  size_t sort_tmp_bytes, scan_tmp_bytes;
  // outputs
  int32_t* out_root_index;      // [T][2n-3]
  int32_t* out_slot_index;      // [T][2(2n-3)][3]
  int32_t* out_counts;          // [3]
  uint32_t* out_split_bits;     // [root_capacity][W]
  int32_t* out_pcsp_clades;     // [pcsp_capacity][3]
  int32_t* out_parent_range;    // [pcsp_capacity][2]
  int32_t* out_pcsp_parent;     // [pcsp_capacity]
};
size_t sbn_index_sort_tmp_bytes(size_t occurrences);
size_t sbn_index_scan_tmp_bytes(size_t occurrences);
int launch_sbn_index(const SbnIndexArgs& a, hipStream_t s);  // (after the split table; nonzero: rocPRIM refused)
struct SbnProbArgs {
  int n, T, tpw;
  int P;                        // parameters: rootsplits + PCSPs (the sentinel)
  int uniform;                  // 1: every rooting has weight 1 (the counts of simple-average training)
  int require_support;          // 1: a sentinel in a tree is an error (training)
  const int32_t* parent_ids;    // [T][2n-3]
  const int32_t* root_index;    // [T][2n-3]
  const int32_t* slot_index;    // [T][2(2n-3)][3]
  const double* theta;          // [P] normalised log parameters
  const double* weights;        // [T] or nullptr
  int32_t* status;
  char* store;
  double* usage;                // [T][7 (2n-3)] log usage of every entry (roots, then slots), or nullptr
  uint32_t *keys, *keys2, *vals, *vals2;  // [T 7 (2n-3)] the accumulation's sort
  void* sort_tmp;
  size_t sort_tmp_bytes;
  double* out_rooting;          // [T][2n-3]
  double* out_log_q;            // [T]
  double* out_counts;           // [P] or nullptr
};
size_t sbn_prob_sort_tmp_bytes(size_t entries, int P);
void sbn_prepare(int n, int tpw);  // the large-LDS opt-in (before a graph capture)
int launch_sbn_log_prob(const SbnProbArgs& a, hipStream_t s);
// out[j] = in[j] - logsumexp(block of j): block 0 is [0, S), block b > 0 is parent_range[b-1]
void launch_sbn_normalize(int S, int parents, const int32_t* parent_range, const double* in, double* out,
                          hipStream_t s);
// status if an entry is NaN or +inf
void launch_sbn_check_params(int P, const double* theta, int32_t* status, hipStream_t s);
// out[j] = log(exp(a[j]) + exp(b[j] + shift)) (b nullptr: a[j] + shift)
void launch_sbn_combine(int P, const double* a, const double* b, double shift, double* out, hipStream_t s);
// *out = sum_t w_t log_q[t] (+ sum_j exp(log_m[j]) theta[j] if log_m), in ascending order by one wave
void launch_sbn_score(int T, const double* weights, const double* log_q, int P, const double* log_m,
                      const double* theta, double* out, hipStream_t s);
// kernels_sbn_vi.hip: the descent table, the sampler and the topology gradient.
// The per-tree kernels (descent: a lane per support tree; sample: a lane per sample) use the node
// arrays above: the same six words per node, the same [word][node][tpw] layout, LDS or `store`.
struct SbnDescentArgs {
  int n, T0, tpw;
  int S, C;
  const int32_t* parent_ids;   // [T0][2n-3]
  const int32_t* root_index;   // [T0][2n-3]
  const int32_t* slot_index;   // [T0][2(2n-3)][3]
  const int32_t* pcsp_parent;  // [C]
  int32_t* status;
  char* store;
  int32_t* out_descent;        // [S + C][2]
};
void launch_sbn_descent(const SbnDescentArgs& a, hipStream_t s);
// The state of a variational fit (mi_vi): one struct in device memory that the
// sampler, the branch-length draw, the branch-length gradient and the optimiser read where a plain
// call takes seed-side arguments by value.  Only vi_finish_kernel writes it.
struct ViState {
  int64_t t, a;            // steps enqueued so far (failed ones included); successful ones
  int64_t first_sample;    // the sample base: sample k of step t is first_sample + t K + k
  int64_t K, anneal_steps; // (constants of the fit)
  double b0, b1;           // beta0^a, beta1^a: one rounded multiply per successful step, from 1
  double step[2], sbn_step;
};
__host__ __device__ inline int64_t vi_sample_base(const ViState& s) { return s.first_sample + s.t * s.K; }
// beta of step t: 1 without annealing, else max(min((t+1) / anneal_steps, 1), 0.001)
__host__ __device__ inline double vi_beta(int64_t t, int64_t anneal_steps) {
  if (anneal_steps <= 0) return 1.0;
  const double b = (double)(t + 1) / (double)anneal_steps;
  return b < 1.0 ? (b > 0.001 ? b : 0.001) : 1.0;
}
struct SbnSampleArgs {
  int n, K, tpw;
  int S, C, parents;
  const int32_t* parent_range;  // [parents][2]
  const int32_t* descent;       // [S + C][2]
  const double* phi;            // [S + C] log parameters, unnormalised
  uint64_t seed;
  int64_t first_sample;
  const ViState* vi;            // a fit's step: first_sample is the state's (else nullptr)
  int32_t* status;
  char* store;
  double* cdf;                  // [S + C]
  double* block_max;            // [parents + 1] the rootsplits' maximum, then every parent's
  int32_t* out_parent_ids;      // [K][2n-3]
  int32_t* out_root_edge;       // [K]
  int32_t* out_params;          // [K][n-1]
  double* out_log_prob;         // [K]
};
void launch_sbn_sample(const SbnSampleArgs& a, hipStream_t s);  // the CDF, then the draws
struct SbnGradientArgs {
  int n, T, P, S, parents;
  int estimator;                // MI_SBN_FACTORS_*
  const int32_t* root_index;    // [T][2n-3]
  const int32_t* slot_index;    // [T][2(2n-3)][3]
  const int32_t* parent_range;  // [parents][2]
  const double* theta;          // [P] normalised
  const double* log_f;          // [T]
  const double* usage;          // [T][7 (2n-3)] log usage, as sbn_walk_kernel leaves it
  uint32_t *keys, *keys2, *vals, *vals2;  // [T 7 (2n-3)]
  void* sort_tmp;
  size_t sort_tmp_bytes;
  double* G;                    // [P] workspace
  double* sums;                 // [2] workspace: log F and sum log_f
  double* out_factors;          // [T]
  double* out_gradient;         // [P]
};
int launch_sbn_gradient(const SbnGradientArgs& a, hipStream_t s);  // (after the walk; nonzero: rocPRIM refused)
void launch_sbn_factors(const SbnGradientArgs& a, hipStream_t s);  // (its first step alone: log_f -> out_factors, through sums)
void sbn_vi_prepare(int n, int tpw);  // the large-LDS opt-in of the two per-tree kernels
// kernels_branch_model.hip: PSP indexing and the log-normal branch-length models.
// E = 2n-3 edges; an index array is [T][R][E], R = 1 (splits) or 3 (rootsplit, down PSP, up PSP);
// an entry outside [0, V) names no variable.
struct PspTableArgs {
  int S, C;
  const int32_t* pcsp_clades;   // [C][3]
  int32_t* out_psp_of_pcsp;     // [C]
  int32_t* out_counts;          // [2] S, V
};
void launch_psp_table(const PspTableArgs& a, hipStream_t s);
struct PspIndexArgs {
  int n, T, S, C, V, R;
  const int32_t* root_index;    // [T][2n-3]
  const int32_t* slot_index;    // [T][2(2n-3)][3]
  const int32_t* psp_of_pcsp;   // [C]
  int32_t* out_index;           // [T][R][2n-3]
};
void launch_psp_index(const PspIndexArgs& a, hipStream_t s);
struct BranchSampleArgs {
  int n, T, R, V;
  const int32_t* index;         // [T][R][2n-3]
  const double* q_params;       // [V][2] mu, sigma
  uint64_t seed;
  int64_t first_sample;
  const ViState* vi;            // a fit's step: first_sample is the state's (else nullptr)
  double prior_rate;
  const double* epsilon_in;     // [T][2n-3] or nullptr
  int32_t* status;
  double* out_bl;               // [T][2n-2]
  double* out_epsilon;          // [T][2n-3]
  double* out_log_q;            // [T]
  double* out_log_prior;        // [T]
};
void launch_branch_sample(const BranchSampleArgs& a, hipStream_t s);
struct BranchGradientArgs {
  int n, T, R, V;
  const int32_t* index;         // [T][R][2n-3]
  const double* q_params;       // [V][2]
  const double* bl;             // [T][2n-2] theta, as the sample call left it
  const double* epsilon;        // [T][2n-3]
  const double* log_q_branch;   // [T]
  const double* log_prior;      // [T]
  const double* branch_gradient;  // [T][2n-1]
  const double* log_likelihoods;  // [T]
  const double* log_q_topology;   // [T] or nullptr
  const double* weights;          // [T] or nullptr
  double beta, prior_rate;
  const ViState* vi;            // a fit's step: beta is the state's (else nullptr)
  int32_t* status;
  double* terms;                // [T][2n-3][2] workspace: c0, c1 of every edge
  uint32_t *keys, *keys2, *vals, *vals2;  // [T R (2n-3)]
  void* sort_tmp;
  size_t sort_tmp_bytes;
  double* out_gradient;         // [V][2]
  double* out_log_f;            // [T]
};
size_t branch_model_sort_tmp_bytes(size_t entries);
int launch_branch_gradient(const BranchGradientArgs& a, hipStream_t s);  // (nonzero: rocPRIM refused)
// kernels_vi_fit.hip: the optimiser of a variational fit and its trace row.
// Element i of the update: 0 .. P-1 the SBN parameters, then the 2 V entries of q_params.
struct ViUpdateArgs {
  int P, V, K;
  int S;                        // variables 0 .. S-1 stand alone on an edge: their sigma must stay positive
  double beta0, beta1, epsilon, decay;
  ViState* state;
  const double* g_sbn;          // [P]
  const double* g_q;            // [V][2]
  const double *log_lik, *log_prior, *log_q_top, *log_q_branch;  // [K]
  double* phi;                  // [P]
  double* q_params;             // [V][2]
  double *m_sbn, *v_sbn;        // [P]
  double *m_q, *v_q;            // [V][2]
  int32_t* block_flags;         // [blocks of 256 elements] workspace
  double* trace;                // [max_steps][6]: the step's row is [t], or nullptr
  int64_t max_steps;
  double* out_row;              // [6] or nullptr: the row once more (mi_vi_update)
};
int vi_update_blocks(int P, int V);
void launch_vi_update(const ViUpdateArgs& a, hipStream_t s);  // check, apply, finish
// kernels_gp.hip: generalized pruning over a subsplit DAG.  A workgroup is one
// wave over a tile of kGpTile patterns; a launch takes the nodes of one level (equal clade size).
// Vectors are [internal node][4][Pp] (Pp: P rounded up to whole tiles), their exponents [..][Pp]:
// true value = stored value x 2^exponent.
constexpr int kGpTile = 64;
constexpr int kGpSums = 5;  // per entry: sum w log l | sum w l'/l | g | H | S
struct GpArgs {
  int n, P, Pp, tiles, G, R, I;          // taxa, patterns, padded patterns, tiles, entries, rootsplits, internal nodes
  double threshold;                      // a vector whose largest entry is below it is rescaled
  const DevModel* model;
  int Cp;                                // row stride of `codes` (distance_code_stride)
  const uint8_t* codes;                  // [distance_code_rows(n)][Cp] tip codes 0..3, 4: all ones (launch_distance_codes)
  const double* weights;                 // [P]
  const double* b;                       // [G]
  const double* q;                       // [G]
  const int32_t* edge;                   // [G][3] parent node, clade, child node (rootsplits: -1, -1, node)
  const int32_t* block_range;            // [nodes][2][2] begin, end
  const int32_t* in_range;               // [nodes][2] begin, end into in_edges
  const int32_t* in_edges;               // entries into a node, ascending
  const int32_t* order;                  // internal nodes by (level, id)
  double* mats;                          // [G][16] P(b_e), row-major
  double* expl;                          // [G][8] e^{lambda_i b_e}, lambda_i (rate included)
  double *phat, *p, *r;                  // [I][2][4][Pp], [I][4][Pp], [I][2][4][Pp]
  int32_t *ephat, *ep, *er;              // [I][2][Pp], [I][Pp], [I][2][Pp]
  double* marg;                          // [Pp] M_p's stored value
  int32_t* emarg;                        // [Pp] its exponent
  double* log_marg;                      // [Pp] log M_p
  double* partial;                       // [G+1][tiles][kGpSums]; row G: the marginal's
  double* sums;                          // [G+1][kGpSums]
  double* matrix;                        // [G][P] log l_e per pattern, or nullptr
};
void launch_gp_matrices(const GpArgs& a, hipStream_t s);
void launch_gp_rootward(const GpArgs& a, int first, int count, hipStream_t s);   // a level of `order`
void launch_gp_marginal(const GpArgs& a, hipStream_t s);
void launch_gp_leafward(const GpArgs& a, int first, int count, hipStream_t s);   // a level of `order`
void launch_gp_leaves(const GpArgs& a, hipStream_t s);                           // the entries into leaves
void launch_gp_finalize(const GpArgs& a, hipStream_t s);
// scatter of the sums: what the calls hand out (any pointer may be nullptr)
void launch_gp_outputs(const GpArgs& a, double* per_gpcsp, double* log_marginal, double* ll_deriv, double* g, double* h,
                       double* s_out, hipStream_t s);
// kernels_gp_hybrid.hip: quartet hybrid marginals over the last populate's vectors.
// desc, per entry: formed | first summand | summands | 0 | then (begin, end) of the rootward list
// (into in_edges, rootsplits skipped) and of the sister, rotated and sorted blocks (entries).
constexpr int kGpHybridDesc = 12;
struct GpHybridArgs {
  int L, F, S, Z;                        // levels, formed entries, summands, gridDim.z of the summand kernel
  int widest;                            // the largest summand count of one entry
  const int32_t* level_range;            // [L][2] first, count into GpArgs::order, ascending level
  const int32_t* desc;                   // [G][kGpHybridDesc]
  const int32_t* formed;                 // [F] the formed entries, ascending
  double *pr, *log_pr;                   // [nodes] Pr(node) and its log
  double* inv;                           // [G] Pr(t) q_e / Pr(s)
  double *z, *a;                         // [G][4][Pp] P(b_e) p(child_e); P(b_e)^T r(t,c) (internal children)
  int32_t *ez, *ea;                      // [G][Pp] their exponents
  double* partial;                       // [S][tiles]
  double* summ;                          // [S]
};
// node probabilities, evolve pass, summands, finalize: hybrid [G], summands [S] or nullptr
void launch_gp_hybrid(const GpArgs& a, const GpHybridArgs& h, double* out_hybrid, double* out_summands, hipStream_t s);
// The matrix-core gradient walks (kernels_walk.hip: second generation, kernels_walk3.hip: third;
// the first, gradient_mfma_kernel, was retired in round 6): all categories of a group of four
// per instruction; they also write the log-likelihood partial sums, so no separate logL pass is
// needed (K > 4: the site likelihoods come from a pass of the log-likelihood kernel).
int gradient_mfma_groups(int K);  // waves per pattern tile (category groups of four)
// subst: analytic substitution gradient statistics appended (kSubstExtra doubles)
int gradient_mfma_width(int n, bool subst = false);  // doubles per (gradient evaluation, tile) of its partial sums
// arena variant of the walks (stored post-order vectors in HBM, LDS slots reused): its slot
// assignment pass, and its HBM need per evaluation
void launch_macro_slots(const MacroEntry* macros_in, MacroEntry* macros_out,
                        const int32_t* macro_count, int n, int T, int32_t* need, int32_t* status,
                        const Switches& sw, hipStream_t s);
size_t gradient_arena_bytes_per_eval(int n, int P, int K);
int device_compute_units();  // of the current device
bool arena_single_launch(size_t lds_bytes, size_t waves);  // all waves resident at once?
int gradient_arena_slots_sure(int n);
int gradient_arena_slots_usual(int n);
// second generation of the same walk (kernels_walk.hip): macro-ordered operand streams
void launch_transition_macro(const TransitionMacroArgs& a, hipStream_t s);
// (sw: MI_PHYLO_WALK_TILES_PER_WAVE, MI_PHYLO_GRADIENT_STORE)
void launch_gradient_walk(const LikArgs& a, int count, bool rescale, bool subst, const Switches& sw, hipStream_t s);
bool gradient_walk_fits(int n, int K, bool rescale);
// lut: the call runs the third-generation (look-up) walk, whose arena variant pays one step earlier;
// store: MI_PHYLO_GRADIENT_STORE (Switches::gradient_store)
bool gradient_walk_use_arena(int store, int n, int K, bool rescale, bool subst, size_t waves = (size_t)-1,
                             bool lut = false, int regs = 0);  // regs: the engine's tile width (0: default)
bool gradient_walk_batches_take_arena(int n, int K, bool lut);  // (large batch, no rescaling, no store forced)
size_t gradient_walk_lds_bytes(int n, int K, bool rescale, bool subst, int regs = 0);
size_t gradient_walk_lds_bytes_for(int n, int K, bool rescale, bool subst, int slots, int regs = 0);
size_t gradient_walk_mats_bytes_per_eval(int n, int K);
const char* gradient_walk_kernel_name();
// kernels_walk3.hip: the third-generation walk (tip children are table look-ups)
size_t gradient_walk_lut_mats_bytes_per_eval(int n);
void launch_transition_lut(const TransitionMacroArgs& a, hipStream_t s);
bool gradient_walk_lut_applies(int K);
// (sw: MI_PHYLO_ARENA_NT, MI_PHYLO_GRADIENT_STORE)
void launch_gradient_walk_lut(const LikArgs& a, int count, bool rescale, const Switches& sw, hipStream_t s);
// The one-launch small call (round 5): tree set-up, model instances and operand records as the
// FIRST workgroups of the walk's launch (four waves per tree), the walk waves wait for their
// tree's hand-off word `ready[t]` (zero before the launch; reduce_finalize clears it again).
// One model instance per tree, one evaluation per tree, trees of at most 64 nodes.
// (a word per 128-byte line: the 78 walk waves of a tree poll their tree's word, and all the
// words of a batch in a handful of lines made ONE memory channel serve every poll of the chip --
// the set-up waves' adds then queued behind them for 6 microseconds)
constexpr int kReadyStride = 32;
struct FusedSetupArgs {
  TreeSetupArgs ts;
  ModelSetupArgs ms;
  double* mmats;     // operand records of gradient evaluation 0 of the launch
  int32_t* ready;    // [T][kReadyStride]
  int setup_blocks;  // 4 T
  int spin_ticks;    // how long a walk wave polls its tree's word (100 MHz ticks; 0: the launcher's default, one second)
  int debug_skip;    // testing: tree debug_skip - 1 never becomes ready (0: off)
  int fence;         // hand-off: 0 none (round 5), 1 L1 + scalar-cache invalidate (default), 2 agent-scope release / acquire
  int colocate;      // set-up waves of a tree on the XCD of its walk waves
  int xcd_base;      // id of the first walk workgroup of the launch that will walk these trees, mod 8 (set by the launchers)
};
bool gradient_walk_lut_fused_applies(int n, int K);
void launch_gradient_walk_lut_fused(const LikArgs& a, const FusedSetupArgs& f, int count, bool rescale,
                                    hipStream_t s);
// The same set-up waves as a launch of their own (round 6): trees, model instances and operand
// records in ONE launch in front of the walk's, for batches beyond the one-launch call's size
// (instead of launch_setup + launch_transition_lut).  f.ready may be nullptr.
void launch_setup_records(const FusedSetupArgs& f, int count, hipStream_t s);
// The same work by a four-wave workgroup per tree: wave 0 builds the tree, wave 1 the model
// instance, then each wave writes a quarter of the tree's operand records (plain stores; the
// ts, ms and mmats members of `f` are read, nothing else).  Four workgroups fit a CU, so a batch
// of 1000 trees is resident at once.  Same conditions as launch_setup_records.
void launch_setup_workgroups(const FusedSetupArgs& f, int count, hipStream_t s);
const char* gradient_walk_lut_kernel_name();
const char* gradient_walk_lut_fused_kernel_name();
// waves per CU the walks' LDS footprint allows for this tree size and category count
int gradient_walk_waves_per_cu(int store, int n, int K);
// Sum of the per-tile partials: ll_sum[e] = sum_i ll_part[e][i] for e < E,
// g_sum[gi][2N] = sum_i g_part[gi][i][2N] for gi < Eg (fixed order: deterministic).
struct ReduceArgs {
  int N, E, Eg, ll_tiles, g_tiles;
  LlCounts ll_used;
  const double* ll_part;
  const double* g_part;
  double* ll_sum;
  double* g_sum;
  // positional partial sums (matrix-core gradient kernel): g_part is
  // [Eg][g_tiles][g_width] indexed by (macro, position, {branch, site}); the schedule maps
  // positions to node ids.  g_width == 0: g_part is [Eg][g_tiles][2N] indexed by node id.
  int g_width, n, T;
  const MacroEntry* macros;
  const int32_t* macro_count;
  // the last `extra` doubles of each positional row are plain sums (analytic substitution
  // gradient: 64 + 4), reduced into x_sum[Eg][extra]
  int extra;
  double* x_sum;
  int keep_offset;  // reduce_finalize_kernel (set by its launcher): where in LDS the reduced sums stay, in doubles
};

// Analytic substitution-model gradient (opt-in): one thread per tree turns the reduced
// statistics into d logL / d (stick-breaking coordinates), 5 rate then 3 frequency ones.
struct SubstGradArgs {
  int T, param_count, rates_off, freqs_off;
  const double* params;   // [T][param_count]
  const DevModel* models; // [T] (one model per tree in this mode)
  const double* x_sum;    // [T][68]
  double* out_subst;      // [T][8]
};
void launch_subst_gradient(const SubstGradArgs& a, hipStream_t s);
constexpr int kSubstExtra = 68;
// Reductions of a variational-inference step over the per-tree results of a gradient call:
//   out_sums[0] = sum_t w_t logL_t, out_sums[1] = sum_t w_t site_gradient_t,
//   out_index_gradient[k] = sum over (t, v) with branch_index[t][v] == k of w_t g[t][v]
// (w_t = 1 without tree_weights; negative indices are skipped), every sum in (t, v) order.
struct ViReduceArgs {
  int T, N, index_count;
  const double* ll;                // [T]
  const double* branch;            // [T][N]
  const double* site;              // [T] or nullptr
  const int32_t* branch_index;     // [T][N]
  const double* tree_weights;      // [T] or nullptr
  double* out_sums;                // [2]
  double* out_index_gradient;      // [index_count]
};
// mi_vi_reduce.hip: stable sort of the entries by index + one ordered sum per run.  The
// workspace (vi_reduce_workspace_bytes) holds the keys, the entry numbers and the sort's
// temporary storage; returns nonzero if the sort could not be enqueued.
size_t vi_reduce_workspace_bytes(long entries, int index_count);
int launch_vi_reduce(const ViReduceArgs& a, void* workspace, size_t workspace_bytes, hipStream_t s);
bool reduce_tiles_fits(int N);
void launch_reduce_tiles(const ReduceArgs& a, hipStream_t s);
void launch_finalize(const FinalizeArgs& a, hipStream_t s);
// both in one launch (a workgroup per tree) for calls with one evaluation per tree
void launch_reduce_finalize(const ReduceArgs& ra, const FinalizeArgs& fa, hipStream_t s);

// ------------------------------------------------------------------------
// 20-state path (kernels_aa.hip): partial-likelihood vectors streamed through HBM in
// 16-pattern matrix-core tiles, one wave per (evaluation, category, pattern block).
// ------------------------------------------------------------------------
constexpr int kAa = 20;              // states
constexpr int kAaTile = 16;          // site patterns per matrix-core tile
constexpr int kAaTipSlack = 512;     // bytes behind the tip-state rows (a workgroup fetches its whole pattern range)
constexpr int kAaTileDoubles = 320;  // one tile of one category: 5 registers x 64 lanes
// one 20x20 matrix as matrix-core A operands: rows 0..15 as five registers x 64 lanes (320
// doubles), rows 16..19 as five blocks of 16 values (a 4x4x4 A operand repeats its 16 values
// in each of the instruction's four blocks: round 5 stores them once) -- 400 doubles, in a
// stride of 512 = four 1 KB pieces of LDS-DMA (until round 5: 10 x 64 = 640, five pieces)
constexpr int kAaPack = 512;
constexpr int kAaPackRows16 = 320;   // offset of the rows-16..19 part
constexpr int kAaTipTable = 21 * 20; // per tip edge and category: column of the matrix per state, 20 = gap
constexpr int kAaPreTiles = 2;       // tiles a wave of the pre-order kernel takes (post-order: 2 or 4)

// The substitution model of a 20-state engine: one eigensystem per engine (an empirical
// model has no free parameters); the per-tree part is the site model in DevModel.
struct AaModel {
  double pi[kAa];
  double lambda[kAa];
  double Q[kAa * kAa];     // row-major, normalised to one expected substitution per unit time
  double V[kAa * kAa];     // eigenvectors
  double Vinv[kAa * kAa];  // inverse eigenvectors
  double Qpack[kAaPack];   // Q as matrix-instruction A operands (the pack layout above)
};

struct AaTransitionArgs {
  int n, N, K;
  int eval_offset, evals;   // this chunk of evaluations (evaluation == tree)
  int gradient;             // also the pre-order matrices
  const AaModel* model;
  const DevModel* models;   // [T]: category rates
  const double* bl_eff;     // [T][N]
  double* matP;             // [evals][n-1][K][kAaPack]  P of internal edges
  double* matPT;            // same: P^T (pre-order propagation)
  double* tipP;             // [evals][n][K][21][20]: tipP[x][i] = P[i][x], x = 20: 1
  double* tipPQ;            // same for P Q (x = 20: 0); internal edges need no P Q: the
                            // derivative uses Q (P L) with the model's one Q operand
};

struct AaWalkArgs {
  int n, N, P, K;
  int tiles;               // 16-pattern tiles, rounded up to a multiple of what one wave takes
  int eval_offset, evals;  // this chunk
  int gradient;            // post-order: every internal vector is kept, indexed by node
  int slots;               // log-likelihood only: vectors are kept by schedule slot
  int ring_slots;          // post-order kernel, both forms (set by the launcher): stack entries a wave keeps in LDS
  int pre_ring_slots;      // pre-order kernel (set by the launcher): parked vectors a wave keeps in LDS
  int ll_stride;           // stride of ll_part per evaluation
  const SchedEntry* sched; // [T][n-1]
  const AaModel* model;
  const DevModel* models;  // [T]
  const double* matP;
  const double* matPT;
  const double* tipP;
  const double* tipPQ;
  const int8_t* tip_states;  // [n][P], 20 = gap
  const double* weights;     // [P]
  double* arena;       // [evals][n-1 | slots][K][tiles][kAaTileDoubles]
  int32_t* exp_cum;    // [evals][n-1 | slots][K][tiles*16]: power of two removed below and at the node
  int32_t* exp_loc;    // [evals][n-1][K][tiles*16]: power of two removed at the node (gradient)
  double* root_val;    // [evals][K][tiles*16]: sum_i pi_i L_root[i] (scaled)
  int32_t* root_exp;   // [evals][K][tiles*16]
  double* root_scale;  // [evals][K][tiles*16]: w_p cw_k 2^(E_k - Emax) / site_p, the root's pre-order weight
  double* ll_part;     // [T][ll_stride]
  double* g_part;      // [evals][K][blocks][N]: per-edge sums of one wave
  double* ll_sum;      // [T]
  double* g_sum;       // [T][2][N]
};

void launch_aa_model_setup(const double* exchangeabilities, const double* freqs, AaModel* model,
                           int32_t* status, const Switches& sw, hipStream_t s);
void launch_aa_transition(const AaTransitionArgs& a, hipStream_t s);
int aa_tiles(int P);                 // padded tile count
int aa_ll_blocks(int P);             // partial log-likelihood sums per evaluation
// (sw: the MI_PHYLO_AA_* launch switches)
void launch_aa_post(const AaWalkArgs& a, const Switches& sw, hipStream_t s);
void launch_aa_root(const AaWalkArgs& a, hipStream_t s);
void launch_aa_pre(const AaWalkArgs& a, const Switches& sw, hipStream_t s);
// entries of the LDS rings the two launchers above will use for these arguments
int aa_post_ring_entries(const AaWalkArgs& a, const Switches& sw);
int aa_post_tiles_per_wave(const AaWalkArgs& a, const Switches& sw);  // 16-pattern tiles a wave of the post-order kernel takes (1, 2 or 4)
int aa_pre_ring_entries(const Switches& sw);
void launch_aa_reduce(const AaWalkArgs& a, hipStream_t s);
const char* aa_post_kernel_name(const Switches& sw);
const char* aa_pre_kernel_name(const Switches& sw);

const char* loglik_kernel_name(const LikArgs& a, bool rescale, int max_slots, const Switches& sw);
const char* gradient_kernel_name();

}  // namespace miphylo
