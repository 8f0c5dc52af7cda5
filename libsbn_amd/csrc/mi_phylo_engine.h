// Private to libmi_phylo.so: the engine object behind include/mi_phylo.h and what its
// translation units share:
//   mi_phylo_engine.cpp       engine creation / destruction, status, profiling, the thin
//                             device-pointer entry points of the C ABI
//   mi_phylo_call.cpp         the call plan (which route a call takes: plan_call), reservation,
//                             the argument-block builders, the 4-state, Hessian, NNI-scan, ancestral-state, placement and SPR-scan call sequences
//   mi_phylo_branch_opt.cpp   branch-length optimisation
//   mi_phylo_nni.cpp          mi_nni_neighbour, the scan's best move on the host (no device code)
//   mi_phylo_spr.cpp          mi_spr_neighbour (no device code)
//   mi_phylo_search.cpp       NNI and SPR moves on the device, the two hill-climbing searches
//   mi_phylo_rell.cpp         per-pattern log-likelihoods (device form), RELL re-summation, tree mixtures
//   mi_phylo_topology_tests.cpp  bootstrap weights drawn on the device, the KH / SH / AU tests
//   mi_phylo_start_trees.cpp  pairwise distances, neighbour joining, starting trees (device forms, reservation)
//   mi_phylo_splits.cpp       split tables, Robinson-Foulds distances (device and host forms, reservation), mi_consensus_tree
//   mi_phylo_sbn.cpp          subsplit Bayesian networks: support and slots, probabilities, normalisation, training
//   mi_phylo_branch_model.cpp PSP indexing and the log-normal branch-length models of a variational step
//   mi_phylo_vi.cpp           the variational fit: its device state, one step, the fit, the optimiser call
//   mi_phylo_gp.cpp           generalized pruning: the subsplit DAG (host), its device object, the sweeps, the optimiser
//   mi_phylo_host_calls.cpp   what runs a host-pointer call (staging, status, shards), the plain entry points
//   mi_phylo_engine_aa.cpp    20-state call sequence
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/mi_phylo.h"
#include "mi_phylo_buffer.h"
#include "mi_phylo_host_arrays.h"
#include "mi_phylo_kernels.h"

namespace miphylo {
void set_last_error(const std::string& msg);
}
using miphylo::fail;
using namespace miphylo;

struct Block {
  std::string name;
  int start, length;
};

inline const char* status_message(int code) {
  switch (code) {
    case kBadParentIds: return "parent id vector is not in the reference's post-order id form";
    case kNotBifurcating: return "expected a bifurcating tree (node.cpp:198,240)";
    case kNotTrifurcatingRoot:
      return "UnrootedTree::Detrifurcate given a non-trifurcating tree.";
    case kGtrFrequencies: return "GTR frequencies do not sum to 1 +/- 0.001!";
    case kGtrRates: return "GTR rates do not sum to 1 +/- 0.001!";
    case kBadRateCount:
      return "The number of rates should be equal to 1 (i.e. strict clock) or equal to the "
             "number of branches.";
    case kTooManySlots: return "internal error: evaluation schedule needs too many LDS slots";
    case kFusedTimeout:
      return "internal error: the walk waves of the one-launch call waited in vain for their "
             "tree's set-up waves (MI_PHYLO_FUSED_SETUP=0 selects the four-launch sequence)";
    case kBadNniMove: return "NNI move is neither -1 nor the code 2 v + i of an inner edge";
    case kBadDistance: return "neighbour joining: a distance is not finite";
    case kBadColumnPattern: return "placement: a column_pattern entry is outside [0, pattern_count)";
    case kBadPendantLength: return "placement: a pendant length is not finite or is negative";
    case kBadSprMove:
      return "SPR move is neither (-1, -1, -1) nor a triple (s, dir, f) that mi_spr_neighbour takes";
    case kSplitCapacity: return "split index: the batch has more distinct splits than split_capacity";
    case kSbnCapacity: return "SBN index: the support has more rootsplits or PCSPs than the capacities";
    case kSbnBadParam: return "SBN log parameters must be finite or -inf";
    case kSbnBadWeight: return "SBN tree weights must be finite and not negative";
    case kSbnOutOfSupport: return "SBN training: a training tree has a rootsplit or PCSP outside the support";
    case kSbnEmptyBlock: return "SBN sample: a sample reached a block whose parameters are all -inf";
    case kSbnBadDescent: return "SBN sample: the descent table or parent_range does not describe a support of this taxon count";
    case kSbnSupportSentinel: return "SBN descent: a support tree has a rootsplit or PCSP outside the support";
    case kBranchModelBadParam:
      return "branch model: an edge's summed sigma must be finite and positive and its summed mu not NaN";
    case kGpTreeBadParam: return "generalized pruning: SBN parameters must be finite and not negative to be sampled from";
    case kGpTreeOutOfDag: return "generalized pruning: a training tree has a subsplit or an entry outside the DAG";
    case kGpTreeEmptyBlock: return "generalized pruning: a sample reached a block whose parameters are all 0";
    case kBootBadWeight: return "bootstrap weights: pattern weights must be non-negative integer site counts";
    case kBootBadTotal: return "bootstrap weights: the pattern weights must sum to N with 1 <= N < 2^31";
    case kBootSitesNotTotal: return "topology tests: sites[0] must equal the sum of the pattern weights";
    case kGpViBadEntry: return "generalized pruning: a node of a tree names no entry of the DAG to take its branch length from";
    default: return "unknown device status";
  }
}

constexpr int kStatusWords = 4;  // code, tree, 1 + tree of a one-launch time-out, spare

// Every resource below releases itself.  The order of an engine's end is the destructor's body
// (mi_phylo_engine.cpp: shards before their front handle, the engine's device made current, its
// stream synchronised) followed by the members in reverse order of declaration: `stream` is
// declared before every buffer, the pinned memory and the events, so it goes last.
struct mi_engine {
  ~mi_engine();
  mi_engine_spec spec;
  int n, N, P, K, tiles, max_slots, ll_stride;
  int s = 4;  // states: 4 (kernels_{loglik,gradient}.hip) or 20 (kernels_aa.hip)
  int param_count, rates_off, freqs_off, shape_off, clock_off;
  std::vector<Block> blocks;
  Stream stream;
  // static device data
  Buffer tip_states, tip_partials, tip_masks, tip_codes, weights;
  Buffer tip_code_tiles;  // tip_codes by pattern tile of the look-up walk (launch_tip_code_tiles), if have_tip_codes and K <= 4
  Buffer tip_tiles;  // tip_masks by pattern tile of the matrix-core log-likelihood kernel (launch_tip_tiles), if have_tip_masks
  bool have_tip_masks = false;  // every tip vector is 0/1: the matrix-core kernel can run
  bool have_tip_codes = false;  // ... and one-hot or all ones: the third-generation walk can run
  // per-call workspace
  Buffer arena_macros, slot_need, tree_scratch, sched, macros, macro_count, bl_eff, models, mats, tip_tables, mmats, mphi, x_sum, ll_part, plv, g_part, site_lik, site_exp, fin_scratch,
      ll_sum, g_sum, status;
  Buffer weibull_x;  // [K][2] {x_k, log x_k} of the Weibull quantiles (once per engine)
  Buffer ready;  // [T] hand-off words of the one-launch small call (zero between calls)
  bool fused_setup = true;  // sw.fused_setup, turned off for good by a time-out (check_status)
  bool fused_timed_out = false;  // check_status found the one-launch call's time-out word set
  int fused_fallbacks = 0;       // host-pointer calls that were run again through four launches
  // 20-state path: the engine's eigensystem and the streamed workspace (the arena is `plv`)
  Buffer aa_model, aa_matP, aa_matPT, aa_tipP, aa_tipPQ, aa_exp_cum, aa_exp_loc,
      aa_root_val, aa_root_exp, aa_root_scale;
  bool aa_reserved_gradient = false;
  PinnedArena pinned;
  Switches sw;  // the MI_PHYLO_* switches as they were when the engine was created
  int tile_regs = 0;  // look-up walk: the engine's tile width (0: default, 4: wide -- engine_tile_regs, at creation)
  // a sharded handle (mi_engine_create_sharded): the per-device / per-shard engines it
  // drives (deleted by its destructor); such a handle owns no device memory itself
  std::vector<mi_engine*> shards;
  int shard_mode = 0;
  std::vector<double> shard_sums;  // per-shard partial results (pattern shards, fused sums)
  // fused reductions (mi_engine_gradients_unrooted_reduced*)
  Buffer red_ll, red_g, red_site, red_sort;
  long red_ws_entries = -1;  // what red_ws_bytes (the sort's workspace size) was computed for
  int red_ws_bits = 0;
  size_t red_ws_bytes = 0;
  // staging for the host-pointer entry points: one block each way per call (run_on_engine)
  Buffer in_pack, out_pack;
  // branch-length optimisation (mi_engine_optimize_branch_lengths_unrooted*)
  Buffer opt_ws;                // trial points, kept derivatives, packed inputs, maps, counters
  PinnedWord opt_word;          // pinned: the active count read at a check point
  // NNI moves and the NNI search (mi_engine_nni_{apply,search}_unrooted*)
  Buffer nni_apply_ws;   // the apply kernel's working arrays of trees too large for LDS
  Buffer nni_search_ws;  // the pair of tree buffers, a round's results, packed inputs, maps, counters
  // per-pattern log-likelihoods and RELL (mi_engine_pattern_log_likelihoods_unrooted*, mi_engine_rell*)
  Buffer pattern_blank;   // [P] 1 where every tip vector of the pattern is all ones (once per engine: launch_pattern_blank)
  Buffer pattern_ll_out;  // [T] the call's log-likelihoods when the caller wants none (mi_engine_reserve)
  Buffer rell_ws;         // [B][T] product (when the caller wants none) | row maxima, 1 / denominators [B] each | counts [T] (mi_engine_reserve_rell)
  Buffer rell_s;          // the fused host call: [T][P] per-pattern values nobody downloads
  // bootstrap weights and the KH / SH / AU tests (mi_engine_bootstrap_weights*, mi_engine_topology_tests*)
  Buffer boot_ws;         // prefix sum [P+1] | N | the global form's histogram rows (mi_engine_reserve_bootstrap_weights)
  Buffer topo_ws;         // a block's weights [B][P] and product [B][T] | row statistics [B] x 3 | per-tree rows (mi_engine_reserve_topology_tests)
  // starting trees (mi_engine_pairwise_distances*, mi_engine_neighbour_joining*, mi_engine_starting_trees_unrooted*)
  Buffer dist_codes;   // [n4][Pp] one-byte tip codes of the count kernel (once per engine: launch_distance_codes)
  Buffer dist_model;   // the call's one model instance
  Buffer dist_counts;  // a chunk of replicates' counts [chunk][n(n-1)/2][16]
  Buffer dist_matrix;  // starting trees: [B][n][n] distances nobody asked for
  Buffer nj_ws;        // neighbour joining: the working sets of matrices too large for LDS
  // placement (mi_engine_placement_unrooted*)
  Buffer place_bl;     // [T][N] halved effective lengths | [T][G+1] the pendant lengths, a row per tree
  Buffer place_half;   // [T][N-1][K][16] P(r_k t_e / 2) by node id
  Buffer place_pend;   // [T][G][K][16] P(r_k l_g)
  Buffer place_table;  // [trees of a table launch][2n-3][G][5][tiles*64]: counts against plv_budget
  // the SPR neighbourhood scan (mi_engine_spr_scan_unrooted*)
  Buffer spr_bl;    // [T][N] halved effective lengths
  Buffer spr_half;  // [T][N-1][K][16] P(r_k t_e / 2) by node id
  Buffer spr_ws;    // per tree of a launch: second arena, exponents, L_p, per-tile partial table: counts against plv_budget
  Buffer spr_path;  // [waves] the regraft waves' paths: messages and their exponents
  // SPR moves and the SPR search (mi_engine_spr_{apply,search}_unrooted*)
  Buffer spr_apply_ws;   // the apply kernel's working arrays of trees too large for LDS
  Buffer spr_search_ws;  // the pair of tree buffers, a round's results, packed inputs, maps, counters
  // split tables and Robinson-Foulds distances (mi_engine_split_index*, mi_engine_rf_distances*)
  Buffer split_ws;     // occurrences: bitsets [O][W] | hashes, then flags and ranks [O] 8 bytes | slots [O] | the table: owner, first, trees [slots] each | the scan's temporary storage
  Buffer split_store;  // tree_splits_kernel's working bitsets of trees too large for LDS
  Buffer split_sort;   // the statistics' sort: keys, values, sorted keys, sorted values [O] each | rocPRIM's temporary storage
  // subsplit Bayesian networks (mi_engine_sbn_*)
  Buffer sbn_index_ws;  // the index call: the batch's split table | PCSP occurrences, the two tables, the sort and the scan
  Buffer sbn_prob_ws;   // log_prob / normalize / train: normalised parameters | usages | the accumulation's sort | training vectors
  Buffer sbn_store;     // the per-tree kernels' node arrays of trees too large for LDS
  // PSP indexing and the branch-length models (mi_engine_psp_*, mi_engine_branch_model_*)
  Buffer branch_ws;     // the gradient call: every edge's two terms | the accumulation's sort
  // a variational fit (mi_vi, mi_phylo_vi.cpp): set while mi_vi_step_device enqueues, so that the
  // sampler, the branch-length draw and its gradient read first_sample and beta from the fit's state
  const ViState* vi_state = nullptr;
  Buffer deroot_ws;    // de-rooting (mi_engine_reserve_deroot): per-tree node words
  Buffer rf_ws;        // a batch's sorted lists: lengths [T][2n-3] | indices [T][2n-3] | counts [T]
  size_t plv_budget = (size_t)8 << 30;  // sw.plv_bytes if set; 20 states: reduced by aa_reserve's back-offs
  // kernel timing (bench.py)
  std::vector<Event> prof_events;  // kProfEvents per call: [begin, end, mark 0..4]
  int prof_capacity = 0, prof_used = 0;
  bool prof_phases = false;   // also record the phase marks (mi_engine_profile_begin_phases)
  int prof_first_launch_evals = 0;  // evaluations in the first walk launch of the last call
  // last-call info
  const char* dominant = "";
  std::string last_path;  // mi_engine_last_call_path
  int64_t last_evals = 0, last_grad_evals = 0;
  int status_tree_offset = 0;  // a shard's first tree in the caller's batch (error messages)
  int last_walk_launches = 1;  // chunks of evaluations the last call's walk kernels ran over
  int aa_backoffs = 0;         // times the 20-state arena budget was reduced (aa_reserve)
};


// Events per profiled call: the pair around the dominant kernel(s) (all launches of a chunked
// call) and, when phases are asked for, five marks: call start | first walk launch starts |
// its post-order part done | its pre-order / main part done | call end.
constexpr int kProfEvents = 7;
inline hipEvent_t prof_event(mi_engine* e, int which) {
  return e->prof_events[(size_t)kProfEvents * e->prof_used + which];
}
#define PROF_MARK(e, on, which, s)                                   \
  do {                                                               \
    if (on) HIP_TRY(hipEventRecord(prof_event(e, 2 + (which)), s)); \
  } while (0)

// ---- the call plan (mi_phylo_call.cpp) ----
// Everything the engine decides about ONE call before it enqueues anything: the evaluation
// shape, the kernel family and its store, which set-up form runs, which passes run and who
// fills the tip tables.  plan_call is the only place these are decided; reservation
// (reserve, reserve_hessian), the argument-block builders, the call sequences and the path
// string (plan_path) read the plan -- so a reserve cannot guess differently from the call it
// reserves for (and leave that call to allocate inside a hipGraph capture).
enum CallKind { kLogLikCall, kGradientCall, kHessianCall, kNniCall, kAncestralCall, kPlacementCall, kSprCall };
enum WalkStore { kStoreHbm = 0, kStoreLds = 1, kStoreArena = 2 };  // (LikArgs::store: 0 = not a matrix-core walk)
struct CallPlan {
  CallKind kind;
  int T;
  bool rescaling, rooted;
  // evaluation shape (EvalMap, mi_phylo_kernels.h): evaluations, gradient evaluations, model instances
  int E, Eg, M, models_per_tree;
  bool gtr, site_fused, site_separate;
  // the gradient / Hessian kernel family and its store
  bool mfma;        // a matrix-core walk (else, for gradient and Hessian calls: the HBM-streamed kernel)
  bool walk3;       // ... of the third generation (look-up walk, kernels_walk3.hip)
  WalkStore store;  // where a walk keeps its stored vectors (kStoreHbm: no walk runs)
  int groups;       // waves per pattern tile (category groups of four)
  int tile_regs;    // look-up walk: tile width of this call (0: the default)
  int g_tiles;      // gradient partial sums per gradient evaluation
  bool analytic;    // analytic substitution gradient (opt-in) instead of finite differences
  bool light;       // GTR gradient call nobody reads the substitution / site gradient of
  bool fuse_setup;     // set-up rides in the walk's launch (the one-launch call)
  bool setup_records;  // set-up and operand records in one launch in front of the walk's (quarter-waves)
  bool setup_wg;       // ... by a four-wave workgroup per tree (at most one of the three is set)
  bool need_slots;     // the schedule gets LDS slots: a log-likelihood (or HBM Hessian) kernel walks it
  bool fd_pass, site_pass;  // the 16 finite-difference passes / the perturbed-model site pass run
  bool loglik_runs;         // a log-likelihood kernel runs at all
  bool loglik_is_valu;      // ... the VALU one (else the matrix-core one)
  bool pattern_ll;          // a log-likelihood call that also hands out the per-pattern values (its kernels' PATTERN_LL variant)
  bool need_tip_tables;     // the transition launch fills the per-state tip tables (VALU log-likelihood kernel)
  // reservation only: what does not follow from this call alone
  size_t mmats_bytes_per_eval;  // macro-ordered matrices of either walk generation this engine can take
  bool reserve_arena;           // some call of this engine (other rescaling / batch size) takes the arena
  bool hand_off_words;          // the one-launch call may run on this engine: `ready` is kept
  const char* dominant;  // the dominant kernel's name
};
// One engine call with every pointer a device pointer (what the *_device entry points build).
struct DeviceCall {
  bool gradient = false, rooted = false, with_jacobian = false, rescaling = false;
  int T = 0;
  const int32_t* parent_ids = nullptr;
  const double* bl = nullptr;
  const double* params = nullptr;
  const double* rates = nullptr;
  const int32_t* rate_counts = nullptr;
  const double* heights = nullptr;
  const double* bounds = nullptr;
  const double* ratios = nullptr;
  double* out_ll = nullptr;
  double* out_branch = nullptr;
  double* out_ratios = nullptr;
  double* out_clock = nullptr;
  double* out_site = nullptr;
  double* out_subst = nullptr;
  // branch-length Hessian call (run_hessian_device): out_ll / out_branch may be nullptr there
  double* out_hess = nullptr;
  double* out_gsq = nullptr;
  // NNI neighbourhood scan (run_nni_device): out_ll / out_best may be nullptr there
  double* out_nni = nullptr;    // [T][N][2]
  int32_t* out_best = nullptr;  // [T]
  // per-pattern log-likelihoods (a log-likelihood call; out_ll may be nullptr there)
  double* out_pattern_ll = nullptr;  // [T][P]
  // ancestral states (run_ancestral_device): all but out_anc_state, and out_ll, may be nullptr there
  double* out_anc_state = nullptr;  // [T][n-2][P][4]
  int8_t* out_anc_map = nullptr;    // [T][n-2][P]
  double* out_anc_cat = nullptr;    // [T][P][K]
  double* out_anc_rate = nullptr;   // [T][P]
  double* out_anc_tip = nullptr;    // [T][n][P][4]
  // placement (run_placement_device): all outputs but out_place_edge_ll, and out_ll, may be nullptr
  int Q = 0, C = 0, G = 0;                // queries, columns, pendant lengths
  const int8_t* query_states = nullptr;   // [Q][C]
  const int32_t* column_pattern = nullptr;  // [C]
  const double* column_weights = nullptr;   // [C] or nullptr
  const double* pendant_lengths = nullptr;  // [G]
  double* out_place_edge_ll = nullptr;    // [T][Q][2n-3]
  int8_t* out_place_pendant = nullptr;    // [T][Q][2n-3]
  int32_t* out_place_best = nullptr;      // [T][Q]
  double* out_place_lwr = nullptr;        // [T][Q][2n-3]
  double* out_place_tables = nullptr;     // [T][2n-3][G][5][P]
  // the SPR scan (run_spr_device): out_spr_target and out_spr_delta are required
  int spr_radius = 0;                     // 0: every move
  int32_t* out_spr_target = nullptr;      // [T][2n-3][2]
  double* out_spr_delta = nullptr;        // [T][2n-3][2]
  int32_t* out_spr_move = nullptr;        // [T][3]
  double* out_spr_table = nullptr;        // [T][2n-3][2][2n-3]
  // ... as one pass of the branch-length optimisation: the batch size the kernel and its store
  // are chosen for (the whole batch's, so that a tree's results do not depend on how many
  // trees are still active); 0: T
  int route_T = 0;
};
// (the defaults: what reservation plans for -- every optional output wanted)
CallPlan plan_call(const mi_engine* e, CallKind kind, int T, bool rescaling, int route_T = 0,
                   bool rooted = false, bool want_site = true, bool want_subst = true);
inline CallPlan plan_call(const mi_engine* e, CallKind kind, const DeviceCall& d) {
  CallPlan p = plan_call(e, kind, d.T, d.rescaling, d.route_T, d.rooted, d.out_site != nullptr, d.out_subst != nullptr);
  p.pattern_ll = kind == kLogLikCall && d.out_pattern_ll != nullptr;
  return p;
}
std::string plan_path(const mi_engine* e, const CallPlan& p);  // mi_engine_last_call_path
bool walk3_possible(const mi_engine* e);  // (engine creation: the look-up walk's pre-tiled tip codes)
int engine_tile_regs(const mi_engine* e);  // (engine creation: decided once, kept in e->tile_regs)
int reserve(mi_engine* e, const CallPlan& p);
int reserve_hessian(mi_engine* e, const CallPlan& p);
int reserve_hessian_calls(mi_engine* e, int T);  // of either rescaling setting (mi_engine_reserve_hessian)
// set-up blocks every call sequence fills the same way (20 states: with a plan that only says need_slots)
TreeSetupArgs tree_setup_args(const mi_engine* e, const DeviceCall& d, const CallPlan& p);
ModelSetupArgs model_setup_args(const mi_engine* e, const DeviceCall& d, const CallPlan& p);
FinalizeArgs finalize_args(const mi_engine* e, const DeviceCall& d);  // what comes from the engine and the call
int run_device(mi_engine* e, hipStream_t s, const DeviceCall& d);
int run_hessian_device(mi_engine* e, hipStream_t s, const DeviceCall& d);
int reserve_nni_calls(mi_engine* e, int T);  // of either rescaling setting (mi_engine_reserve_nni_scan)
int run_nni_device(mi_engine* e, hipStream_t s, const DeviceCall& d);
int reserve_ancestral_calls(mi_engine* e, int T);  // of either rescaling setting (mi_engine_reserve_ancestral)
int run_ancestral_device(mi_engine* e, hipStream_t s, const DeviceCall& d);
// placement: what both entry points refuse before any device work; the workspace
// of a call of T trees and G pendant lengths, of either rescaling setting; the call itself
int check_placement_shape(const mi_engine* e, int Q, int C, int G);
int reserve_placement_calls(mi_engine* e, int T, int G);
int run_placement_device(mi_engine* e, hipStream_t s, const DeviceCall& d);
// the SPR scan: what both entry points refuse before any device work; the
// workspace of a call of T trees, of either rescaling setting and any radius; the call itself
int check_spr_shape(const mi_engine* e, int radius);
int reserve_spr_calls(mi_engine* e, int T);
int run_spr_device(mi_engine* e, hipStream_t s, const DeviceCall& d);
// the scan's best move from a tree's delta [N][2] (what the finalize kernel does; pattern shards)
int32_t nni_best_move(int n, const double* delta);

// ---- mi_phylo_branch_opt.cpp ----
struct BranchOptCall {
  int T = 0;
  bool rescaling = false;
  const int32_t* parent_ids = nullptr;
  const double* start = nullptr;
  const double* params = nullptr;
  const mi_branch_opt_options* options = nullptr;
  double* out_bl = nullptr;
  double* out_ll = nullptr;
  double* out_g = nullptr;      // may be null
  double* out_h = nullptr;      // may be null
  int32_t* out_iters = nullptr;  // may be null
  int32_t* out_status = nullptr;
  // as one round of the NNI search: the batch size the Hessian passes' route is chosen for (0: T)
  int route_T = 0;
};
extern const mi_branch_opt_options kBranchOptDefaults;
int reserve_branch_opt(mi_engine* e, int T);
int check_branch_opt_options(const mi_branch_opt_options& o);
int run_branch_opt_device(mi_engine* e, hipStream_t s, const BranchOptCall& c);

// ---- mi_phylo_engine.cpp ----
extern const char kShardedDeviceCall[], kHessian4State[], kNni4State[], kPatternLl4State[], kAncestral4State[], kPlacement4State[], kSpr4State[];
int check_status(mi_engine* e, hipStream_t s);
inline hipStream_t pick_stream(mi_engine* e, void* stream) {
  return stream ? static_cast<hipStream_t>(stream) : e->stream;
}
// A sharded handle: one(shard, its share of `tree_count` trees) for every shard that has trees
// (pattern shards: every shard gets all of them).
template <typename F>
int for_each_shard(mi_engine* e, int tree_count, F one) {
  const int D = (int)e->shards.size();
  for (int i = 0; i < D; i++) {
    int32_t b = 0, c = tree_count;
    if (e->shard_mode == MI_SHARD_TREES) mi_shard_range(tree_count, D, i, &b, &c);
    if (c > 0 && one(e->shards[i], c)) return 1;
  }
  return 0;
}

// ---- mi_phylo_host_calls.cpp: what every host-pointer entry point is run by ----
// A host-pointer call lists its arrays once (HostArray: mi_phylo_host_arrays.h) and says how its
// device work is enqueued, given their device addresses.  Staging (one copy each way), the one
// synchronisation with its status check and the shards of a handle are driven by the lists.
struct HostCall {
  int T = 0;  // trees (what per-tree arrays are counted in)
  std::vector<HostArray> in, out;
  // enqueue the device work on e->stream; the lists are the call's own, with `dev` filled in
  std::function<int(mi_engine* e, int T, const HostArray* in, const HostArray* out)> enqueue;
  bool retry = false;       // a one-launch time-out: run again through the four-launch sequence
  bool one_by_one = false;  // tree shards run shard after shard (the work synchronises its device)
  bool deliver_on_error = false;  // an error of the status words: the outputs are handed over all the same
};
// A host form that takes NULL for an output its device form requires: the output is made all the same, into host
// memory of the call's that nobody reads.
struct Unwanted {
  std::vector<std::vector<char>> blocks;
  template <typename U>
  U* operator()(U* wanted, size_t count) {
    if (wanted) return wanted;
    blocks.emplace_back(count * sizeof(U));
    return reinterpret_cast<U*>(blocks.back().data());
  }
};
int run_host_call(mi_engine* e, HostCall& c);   // on an engine, or dealt to the shards of a handle
int run_on_engine(mi_engine* e, HostCall& c);   // on this engine
// (calls that need no alignment: a sharded handle of either kind lets its first shard take them)
inline mi_engine* first_engine(mi_engine* e) { return e->shards.empty() ? e : e->shards[0]; }
// the three inputs every tree call begins its list with
enum { kInParent, kInBl, kInParams, kTreeInputs };
inline std::vector<HostArray> tree_inputs(const mi_engine* e, const int32_t* parent_ids, const double* bl,
                                          const double* params, bool rooted = false) {
  const size_t np = rooted ? 2 * e->n - 2 : 2 * e->n - 3;
  return {per_tree(parent_ids, np), per_tree(bl, np + 1),
          per_tree(e->param_count > 0 ? params : nullptr, e->param_count)};
}
// (an engine without parameters still hands the kernels a valid pointer)
inline const double* params_on_device(const mi_engine* e, const HostArray* in) {
  return in[kInParams].dev ? in[kInParams].at<const double>() : e->in_pack.as<const double>();
}

// ---- mi_phylo_rell.cpp ----
// the workspace of a RELL call over B replicates and T trees (mi_engine_reserve_rell)
int reserve_rell(mi_engine* e, int B, int T);
// enqueue the product, the row pass and the column pass; every pointer a device pointer
int run_rell_device(mi_engine* e, hipStream_t s, int B, int T, int P, const double* pattern_ll, const double* weights,
                    double* out_c, int32_t* out_best, double* out_bp, double* out_elw);

// ---- mi_phylo_start_trees.cpp ----
// One call of the starting-tree family with every pointer a device pointer.  weights nullptr:
// one replicate, the engine's pattern weights.
struct PairDistanceCall {
  int B = 0;
  const double* weights = nullptr;  // [B][P]
  const double* params = nullptr;   // [param_count]
  const mi_distance_options* options = nullptr;
  double* out_dist = nullptr;       // [B][n][n]
  double* out_counts = nullptr;     // [B][n(n-1)/2][16] or nullptr
  int8_t* out_status = nullptr;     // [B][n(n-1)/2] or nullptr
};
extern const mi_distance_options kDistanceDefaults;
extern const char kDistance4State[], kDistancePatternShards[];
int distance_options(const mi_distance_options* in, mi_distance_options* out);  // defaults filled in, checked
int check_distance_call(const mi_engine* e, int B);  // what every entry point of calls 1 and 3 checks first
int run_pair_distances_device(mi_engine* e, hipStream_t s, const PairDistanceCall& c);
int run_nj_device(mi_engine* e, hipStream_t s, int B, int n, const double* dist, double tmin, double tmax,
                  int32_t* out_parent_ids, double* out_bl);
int run_start_trees_device(mi_engine* e, hipStream_t s, const PairDistanceCall& c, int32_t* out_parent_ids,
                           double* out_bl);

// ---- mi_phylo_splits.cpp ----
// One split-table call with every pointer a device pointer.
struct SplitIndexCall {
  int T = 0, n = 0, capacity = 0;
  const int32_t* parent_ids = nullptr;  // [T][2n-3]
  const double* bl = nullptr;           // [T][2n-2] or nullptr
  const double* weights = nullptr;      // [T] or nullptr
  int32_t* out_index = nullptr;         // [T][2n-1]
  int32_t* out_count = nullptr;         // [1]
  uint32_t* out_bits = nullptr;         // [capacity][W]
  int32_t* out_first = nullptr;         // [capacity]
  int32_t* out_trees = nullptr;         // [capacity]
  double* out_stats = nullptr;          // [capacity][3] or nullptr
};
int run_split_index_device(mi_engine* e, hipStream_t s, const SplitIndexCall& c);
int run_rf_device(mi_engine* e, hipStream_t s, int T, int n, const int32_t* split_index, const double* bl,
                  int32_t* out_rf, double* out_bs);

// mi_phylo_engine_aa.cpp
int aa_engine_init(mi_engine* e, const double* exchangeabilities, const double* frequencies);
int aa_reserve(mi_engine* e, int T, bool gradient);
int aa_run_device(mi_engine* e, hipStream_t s, const DeviceCall& d);
