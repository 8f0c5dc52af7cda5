// C++ adapter with the public shape of libsbn's Engine (src/engine.hpp:26-54) on
// top of the C ABI (include/mi_phylo.h).  Header-only; links against
// libmi_phylo.so (+ libmi_phylo_host.so for the tree / site-pattern types).
//
//   reference                               here
//   EngineSpecification  engine.hpp:20-24   mihost::EngineSpecification
//   PhyloModelSpecification phylo_model.hpp:13-17   mihost::PhyloModelSpecification
//   PhyloGradient        tree_gradient.hpp:10-19    mihost::PhyloGradient
//   {Unrooted,Rooted}TreeCollection         std::vector<FlatTree> / <RootedFlatTree>
//   EigenMatrixXdRef (row-major)            mihost::ParamMatrix
// Errors are std::runtime_error, like Failwith (src/sugar.hpp:67-78).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../../include/mi_phylo.h"
#include "mi_host.hpp"

namespace mihost {

struct PhyloModelSpecification {
  std::string substitution_, site_, clock_;
};

struct EngineSpecification {
  // The reference makes thread_count_ FatBeagle instances and deals the trees of a call to
  // them (engine.cpp:23-27, fat_beagle.hpp:119-149).  Here the executors are GPUs: the trees
  // of a call are dealt, in contiguous blocks, to min(thread_count_, visible devices) devices
  // driven by ONE handle (mi_engine_create_sharded); on a one-GPU machine any thread count
  // gives one engine.  device_shards_ overrides that (testing: several logical shards).
  size_t thread_count_;
  std::vector<int> beagle_flag_vector_;  // accepted and ignored
  bool use_tip_states_;
  std::vector<int32_t> device_shards_ = {};
};

using GradientMap = std::map<std::string, std::vector<double>>;
struct PhyloGradient {
  double log_likelihood_ = 0.;
  GradientMap gradient_;
};
// Engine::BranchHessians, per tree: [2n-1] each (an extension, include/mi_phylo.h)
struct BranchHessian {
  double log_likelihood_ = 0.;
  std::vector<double> gradient_, hessian_, gradient_sq_;
};

// Engine::NniScan, per tree (an extension, include/mi_phylo.h): delta_[2 v + i] = logL(neighbour i
// of inner edge v) - logL(tree), [2 (2n-1)] by node id, 0 where v is no inner edge; best_move_ =
// 2 v + i of the largest delta (-1: no inner edge)
struct NniNeighbourhood {
  double log_likelihood_ = 0.;
  std::vector<double> delta_;
  int32_t best_move_ = -1;
};

// Engine::PatternLogLikelihoods (an extension, include/mi_phylo.h): log_likelihoods_ [T] and the
// unweighted per-pattern values [T][P], row-major
struct PatternLogLikelihood {
  std::vector<double> log_likelihoods_, pattern_log_likelihoods_;
};

// Engine::RellBootstrap (an extension, include/mi_phylo.h): the per-pattern values [T][P], the
// replicate log-likelihoods [B][T], the best tree per replicate [B] (lowest index among equals),
// bootstrap proportions and expected-likelihood weights [T]
struct RellBootstrapResult {
  std::vector<double> log_likelihoods_, pattern_log_likelihoods_, replicate_log_likelihoods_;
  std::vector<int32_t> best_tree_;
  std::vector<double> bootstrap_proportion_, expected_likelihood_weight_;
};

// Engine::TopologyTests (an extension, include/mi_phylo.h): the trees' log-likelihoods [T] and
// per-pattern values [T][P], the table [T][MI_TOPOLOGY_COLUMNS] (per tree: L | L[best] - L | bp |
// elw | p_KH | p_SH | p_AU | d | c | rss | usable scales), the replicates every tree won per block
// [K][T], the column means of block 0 [T], and the blocks' sites and replicates [K]
struct TopologyTestsResult {
  std::vector<double> log_likelihoods_, pattern_log_likelihoods_, table_;
  std::vector<int32_t> counts_;
  std::vector<double> column_mean_;
  std::vector<int64_t> sites_;
  std::vector<int32_t> replicates_;
};

// Engine::PairwiseDistances (an extension, include/mi_phylo.h): distances_ [B][n][n] (symmetric,
// zero diagonal), the substitution counts pair_counts_ [B][n(n-1)/2][16] of the pairs in
// lexicographic (i, j) order and the solver's status per pair [B][n(n-1)/2] (MI_DISTANCE_*)
struct PairwiseDistanceResult {
  std::vector<double> distances_, pair_counts_;
  std::vector<int8_t> pair_status_;
};

// Engine::NeighbourJoining / Engine::StartingTrees (extensions, include/mi_phylo.h): per matrix /
// replicate the tree in the form every unrooted call takes, parent_ids_ [B][2n-3] and
// branch_lengths_ [B][2n-2], and (StartingTrees) the distances_ [B][n][n] they were joined from
struct StartingTreeResult {
  std::vector<int32_t> parent_ids_;
  std::vector<double> branch_lengths_, distances_;
};

// Engine::SplitIndex (an extension, include/mi_phylo.h): the distinct splits of a batch of unrooted
// trees numbered by first occurrence; split_index_ [T][2n-1], and per split bits_ [S][W], first_ [S],
// trees_ [S] and stats_ [S][3] (sum w, sum w l, sum w l^2 over the trees that hold it)
struct SplitTable {
  size_t taxon_count_ = 0, split_count_ = 0;
  std::vector<int32_t> split_index_, first_, trees_;
  std::vector<uint32_t> bits_;
  std::vector<double> stats_;
};

// Engine::SbnIndex (an extension, include/mi_phylo.h): the subsplit support of the first
// support_tree_count_ trees of a batch and the slots of all its trees.  root_index_ [T][2n-3],
// slot_index_ [T][2(2n-3)][3]; per rootsplit bits_ [S][W]; per PCSP pcsp_clades_ [C][3] (sister,
// focal, child, each 2 split + side) and pcsp_parent_ [C]; per parent parent_range_ [parents][2]
struct SbnSupport {
  size_t taxon_count_ = 0, tree_count_ = 0, support_tree_count_ = 0;
  size_t rootsplit_count_ = 0, pcsp_count_ = 0, parent_count_ = 0;
  std::vector<int32_t> parent_ids_, root_index_, slot_index_, pcsp_clades_, parent_range_, pcsp_parent_;
  std::vector<uint32_t> bits_;
  size_t ParameterCount() const { return rootsplit_count_ + pcsp_count_; }
};

// Engine::SbnLogProb: rooting_log_prob_ [T][2n-3], log_q_ [T] and, asked for,
// log_expected_counts_ [P]
struct SbnProbabilities {
  std::vector<double> rooting_log_prob_, log_q_, log_expected_counts_;
};

// Engine::SbnTrain: normalised log_params_ [P] and the EM score of every iteration run
struct SbnTraining {
  std::vector<double> log_params_, score_history_;
};

// Engine::SbnSample: parent_ids_ [K][2n-3], root_edge_ [K], sampled_params_ [K][n-1] in the order
// of the draws, log_prob_ [K] of the sampled rootings and the cdf_ [P] the draws read
struct SbnSamples {
  std::vector<int32_t> parent_ids_, root_edge_, sampled_params_;
  std::vector<double> log_prob_, cdf_;
};

// Engine::SbnTopologyGradient: gradient_ [P] with respect to the unnormalised parameters, the
// factors_ [K] it was formed with and log_q_ [K]
struct SbnGradient {
  std::vector<double> gradient_, factors_, log_q_;
};

// Engine::PspTable (an extension, include/mi_phylo.h): psp_of_pcsp_ [C] the variable of every PCSP
// that is a PSP (else -1); the variables are the rootsplits, then the PSPs; variable_count_ is also
// the "not present" index.  Engine::PspIndex: [T][rows][2n-3] variable indices
struct PspNumbering {
  size_t rootsplit_count_ = 0, variable_count_ = 0;
  std::vector<int32_t> psp_of_pcsp_;
};

// Engine::BranchModelSample: branch_lengths_ [T][2n-2] (entry 2n-3 is 0), epsilon_ [T][2n-3],
// log_q_ [T], log_prior_ [T]
struct BranchModelDraw {
  std::vector<double> branch_lengths_, epsilon_, log_q_, log_prior_;
};

// Engine::BranchModelGradient: gradient_ [V][2] with respect to (mu, sigma), log_f_ [T]
struct BranchModelGradientResult {
  std::vector<double> gradient_, log_f_;
};

// Engine::ViCreate: a device-resident variational fit (mi_vi, include/mi_phylo.h); it releases
// itself and must not outlive its engine.  ViStateResult: Engine::ViState, the whole state.
class VariationalFit {
 public:
  VariationalFit() = default;
  explicit VariationalFit(mi_vi* handle) : handle_(handle) {}
  VariationalFit(VariationalFit&& o) noexcept : handle_(o.handle_) { o.handle_ = nullptr; }
  VariationalFit& operator=(VariationalFit&& o) noexcept {
    std::swap(handle_, o.handle_);
    return *this;
  }
  VariationalFit(const VariationalFit&) = delete;
  VariationalFit& operator=(const VariationalFit&) = delete;
  ~VariationalFit() { mi_vi_destroy(handle_); }
  mi_vi* Handle() const { return handle_; }
  // n, K, rows, S, C, parent count, V, max_steps, P
  std::array<int32_t, 9> Sizes() const {
    std::array<int32_t, 9> out{};
    if (mi_vi_sizes(handle_, out.data()) != 0) Failwith(mi_last_error());
    return out;
  }

 private:
  mi_vi* handle_ = nullptr;
};
struct ViStateResult {
  std::vector<double> log_params_, q_params_, sbn_moments_, q_moments_;
  std::array<double, 5> scalars_{};    // b0, b1, step_size[0], step_size[1], sbn_step_size
  std::array<int64_t, 3> counters_{};  // t, a, first_sample
};

// Engine::GpCreate: generalized pruning over a subsplit DAG (mi_gp, include/mi_phylo.h); it releases
// itself and must not outlive its engine.
struct GpLikelihoodResult {
  std::vector<double> per_gpcsp_log_likelihood_;  // [G]
  double log_marginal_ = 0.0;
};
struct GpDerivativeResult {
  std::vector<double> ll_derivative_;  // [G][2]
  std::vector<double> gradient_, hessian_, gsq_;  // [G] each
};
struct GpOptimizeResult {
  std::vector<double> branch_lengths_, trace_;
  int32_t evaluations_ = 0, status_ = 0;
};
struct GpHybridRequests {
  std::vector<int32_t> requests_;  // [G][3] formed, first summand, summand count
  std::vector<int32_t> summands_;  // [S][4] the entries (rootward, sister, rotated, sorted) of every summand
  size_t SummandCount() const { return summands_.size() / 4; }
};
struct GpHybridResult {
  std::vector<double> hybrid_;    // [G]
  std::vector<double> summands_;  // [S]
};
// the tree side
struct GpTreeIndexResult {
  std::vector<int32_t> entries_, nodes_;  // [T][2n-1] each; G and -1 mark what the DAG does not hold
};
struct GpTreesResult {  // sampled or enumerated rooted trees
  std::vector<int32_t> parent_ids_;     // [K][2n-2]
  std::vector<int32_t> entries_;        // [K][2n-1]
  std::vector<double> log_q_;           // [K]
  std::vector<double> branch_lengths_;  // [K][2n-1] the GP lengths, 0 at the root
};
struct DerootedTrees {
  std::vector<int32_t> parent_ids_;     // [T][2n-3]
  std::vector<double> branch_lengths_;  // [T][2n-2], empty without input lengths
  std::vector<int32_t> root_edge_;      // [T]
};
struct GpViParticles {  // GeneralizedPruning::ViParticles: the last step's rooted particles of a fit over the DAG
  std::vector<int32_t> parent_ids_;     // [K][2n-2]
  std::vector<int32_t> entries_;        // [K][2n-1]
  std::vector<double> branch_lengths_;  // [K][2n-1], 0 at the root
  std::vector<double> log_likelihoods_, log_q_topology_, log_q_branch_, log_prior_;  // [K] each
};
class GeneralizedPruning {
 public:
  GeneralizedPruning() = default;
  explicit GeneralizedPruning(mi_gp* handle) : handle_(handle) {}
  GeneralizedPruning(GeneralizedPruning&& o) noexcept : handle_(o.handle_) { o.handle_ = nullptr; }
  GeneralizedPruning& operator=(GeneralizedPruning&& o) noexcept {
    std::swap(handle_, o.handle_);
    return *this;
  }
  GeneralizedPruning(const GeneralizedPruning&) = delete;
  GeneralizedPruning& operator=(const GeneralizedPruning&) = delete;
  ~GeneralizedPruning() { mi_gp_destroy(handle_); }
  mi_gp* Handle() const { return handle_; }
  // n, node count, rootsplit count, G, P, words of a clade bitset, levels, tile width
  std::array<int32_t, 8> Sizes() const {
    std::array<int32_t, 8> out{};
    Try(mi_gp_sizes(handle_, out.data()));
    return out;
  }
  size_t EntryCount() const { return static_cast<size_t>(Sizes()[3]); }
  std::vector<double> BranchLengths() const {
    std::vector<double> out(EntryCount());
    Try(mi_gp_get_branch_lengths(handle_, out.data()));
    return out;
  }
  void SetBranchLengths(const std::vector<double>& b) const {
    Try(mi_gp_set_branch_lengths(handle_, b.data(), static_cast<int32_t>(b.size())));
  }
  std::vector<double> SbnParameters() const {
    std::vector<double> out(EntryCount());
    Try(mi_gp_get_sbn_parameters(handle_, out.data()));
    return out;
  }
  void SetSbnParameters(const std::vector<double>& q) const {
    Try(mi_gp_set_sbn_parameters(handle_, q.data(), static_cast<int32_t>(q.size())));
  }
  void Populate() const { Try(mi_gp_populate(handle_)); }
  GpLikelihoodResult Likelihoods() const {
    GpLikelihoodResult out;
    out.per_gpcsp_log_likelihood_.resize(EntryCount());
    Try(mi_gp_likelihoods(handle_, out.per_gpcsp_log_likelihood_.data(), &out.log_marginal_, nullptr, nullptr));
    return out;
  }
  GpDerivativeResult BranchDerivatives() const {
    const size_t G = EntryCount();
    GpDerivativeResult out;
    out.ll_derivative_.resize(2 * G);
    out.gradient_.resize(G);
    out.hessian_.resize(G);
    out.gsq_.resize(G);
    Try(mi_gp_branch_derivatives(handle_, out.ll_derivative_.data(), out.gradient_.data(), out.hessian_.data(),
                                 out.gsq_.data()));
    return out;
  }
  // hybrid: a block whose entries all have a finite hybrid marginal takes softmax(hybrid + log q)
  std::vector<double> EstimateSbnParameters(const bool hybrid = false) const {
    std::vector<double> out(EntryCount());
    Try(hybrid ? mi_gp_estimate_sbn_parameters_hybrid(handle_, out.data())
               : mi_gp_estimate_sbn_parameters(handle_, out.data()));
    return out;
  }
  // the quartet hybrid request of every entry (mi_gp_hybrid_requests)
  GpHybridRequests HybridRequests() const {
    GpHybridRequests out;
    int32_t count = 0;
    Try(mi_gp_hybrid_requests(handle_, nullptr, nullptr, &count));
    out.requests_.resize(3 * EntryCount());
    out.summands_.resize(4 * static_cast<size_t>(count));
    Try(mi_gp_hybrid_requests(handle_, out.requests_.data(), out.summands_.data(), nullptr));
    return out;
  }
  // hybrid [G] (-inf where the request is not fully formed) and every summand [S]
  GpHybridResult HybridMarginals() const {
    GpHybridResult out;
    int32_t count = 0;
    Try(mi_gp_hybrid_requests(handle_, nullptr, nullptr, &count));
    out.hybrid_.resize(EntryCount());
    out.summands_.resize(static_cast<size_t>(count));
    Try(mi_gp_hybrid_marginals(handle_, out.hybrid_.data(), out.summands_.data()));
    return out;
  }
  // ---- trees of the DAG (include/mi_phylo.h) ----
  size_t NodesPerTree() const { return 2 * static_cast<size_t>(Sizes()[0]) - 1; }
  void ReserveTrees(const size_t tree_capacity) const {
    Try(mi_gp_reserve_trees(handle_, static_cast<int32_t>(tree_capacity)));
  }
  uint64_t TopologyCount() const {
    uint64_t out = 0;
    Try(mi_gp_topology_count(handle_, &out));
    return out;
  }
  // rooted trees parent_ids [T][2n-2]: per tree node its entry and its DAG node
  GpTreeIndexResult TreeIndex(const size_t tree_count, const std::vector<int32_t>& parent_ids) const {
    const size_t N = NodesPerTree();
    if (parent_ids.size() != tree_count * (N - 1)) Failwith("TreeIndex: parent_ids is [trees][2n-2].");
    GpTreeIndexResult out;
    out.entries_.resize(tree_count * N);
    out.nodes_.resize(tree_count * N);
    Try(mi_gp_tree_index(handle_, static_cast<int32_t>(tree_count), parent_ids.data(), out.entries_.data(), out.nodes_.data()));
    return out;
  }
  // log q [T] of indexed trees, entries [T][2n-1]
  std::vector<double> TreeLogProb(const std::vector<int32_t>& entries) const {
    const size_t T = entries.size() / NodesPerTree();
    std::vector<double> out(T);
    Try(mi_gp_tree_log_prob(handle_, static_cast<int32_t>(T), entries.data(), out.data()));
    return out;
  }
  std::vector<double> TreeBranchLengths(const std::vector<int32_t>& entries, const double missing_length = 0.0) const {
    const size_t T = entries.size() / NodesPerTree();
    std::vector<double> out(entries.size());
    Try(mi_gp_tree_branch_lengths(handle_, static_cast<int32_t>(T), entries.data(), missing_length, out.data()));
    return out;
  }
  // the rooted TrainSimpleAverage: sets and returns q [G]; tree_weights [T] or empty (1 each)
  std::vector<double> TrainSimpleAverage(const std::vector<int32_t>& entries, const std::vector<double>& tree_weights = {}) const {
    const size_t T = entries.size() / NodesPerTree();
    if (!tree_weights.empty() && tree_weights.size() != T) Failwith("TrainSimpleAverage: tree_weights is [trees] or empty.");
    std::vector<double> out(EntryCount());
    Try(mi_gp_train_simple_average(handle_, static_cast<int32_t>(T), entries.data(),
                                   tree_weights.empty() ? nullptr : tree_weights.data(), out.data()));
    return out;
  }
  // K rooted trees drawn from q: sample k is the Philox stream (seed, first_sample + k)
  GpTreesResult SampleTrees(const size_t sample_count, const uint64_t seed, const int64_t first_sample = 0) const {
    GpTreesResult out = Built(sample_count);
    Try(mi_gp_sample_trees(handle_, static_cast<int32_t>(sample_count), seed, first_sample, out.parent_ids_.data(),
                           out.entries_.data(), out.log_q_.data(), out.branch_lengths_.data(), nullptr));
    return out;
  }
  // trees first .. first + count - 1 of the DAG
  GpTreesResult EnumerateTrees(const int64_t first, const size_t count) const {
    GpTreesResult out = Built(count);
    Try(mi_gp_enumerate_trees(handle_, first, static_cast<int32_t>(count), out.parent_ids_.data(), out.entries_.data(),
                              out.log_q_.data(), out.branch_lengths_.data()));
    return out;
  }

  // A device-resident variational fit over the rooted trees of this DAG (mi_gp_vi_create):
  // log_params [G], q_params [G][2], model_params the one parameter row (empty: the model takes none).
  // options.rows must be 1.  Engine::ViFit, ViState and ViUpdate serve the fit; it must not outlive this object.
  VariationalFit ViCreate(const std::vector<double>& log_params, const std::vector<double>& q_params,
                          const mi_vi_options& options, const std::vector<double>& model_params = {}) const {
    if (q_params.size() % 2) Failwith("ViCreate: q_params is [G][2].");
    mi_vi* fit = nullptr;
    Try(mi_gp_vi_create(handle_, model_params.empty() ? nullptr : model_params.data(), static_cast<int32_t>(log_params.size()),
                        log_params.data(), static_cast<int32_t>(q_params.size() / 2), q_params.data(), &options, &fit));
    return VariationalFit(fit);
  }
  // the last step's rooted particles (mi_gp_vi_particles)
  GpViParticles ViParticles(const VariationalFit& fit) const {
    const size_t K = static_cast<size_t>(fit.Sizes()[1]), N = NodesPerTree();
    GpViParticles out;
    out.parent_ids_.resize(K * (N - 1));
    out.entries_.resize(K * N);
    out.branch_lengths_.resize(K * N);
    for (auto* v : {&out.log_likelihoods_, &out.log_q_topology_, &out.log_q_branch_, &out.log_prior_}) v->resize(K);
    Try(mi_gp_vi_particles(fit.Handle(), out.parent_ids_.data(), out.entries_.data(), out.branch_lengths_.data(),
                           out.log_likelihoods_.data(), out.log_q_topology_.data(), out.log_q_branch_.data(),
                           out.log_prior_.data()));
    return out;
  }

  // options nullptr: tolerance 1e-6, 100 iterations, lengths in [e^-13.9, e^1.1]
  GpOptimizeResult OptimizeBranchLengths(const mi_branch_opt_options* options = nullptr) const {
    GpOptimizeResult out;
    out.trace_.resize(options ? static_cast<size_t>(std::max(options->max_iterations, 1)) : 100);
    Try(mi_gp_optimize_branch_lengths(handle_, options, out.trace_.data(), &out.evaluations_, &out.status_));
    out.trace_.resize(static_cast<size_t>(out.evaluations_));
    out.branch_lengths_ = BranchLengths();
    return out;
  }

 private:
  static void Try(const int32_t rc) {
    if (rc != 0) Failwith(mi_last_error());
  }
  GpTreesResult Built(const size_t count) const {
    const size_t N = NodesPerTree();
    GpTreesResult out;
    out.parent_ids_.resize(count * (N - 1));
    out.entries_.resize(count * N);
    out.log_q_.resize(count);
    out.branch_lengths_.resize(count * N);
    return out;
  }
  mi_gp* handle_ = nullptr;
};

// Engine::RfDistances: rf_ [T][T] and, with branch lengths, branch_score_ [T][T]
struct TreeDistances {
  std::vector<int32_t> rf_;
  std::vector<double> branch_score_;
};

// ConsensusTree: parent_ids_ [m-1] and node_split_ [m] (the table index of each node's edge, -1
// for the root) of the majority-rule consensus, m = n+1 .. 2n-2 nodes
struct ConsensusTreeResult {
  std::vector<int32_t> parent_ids_, node_split_;
};

// Engine::AncestralStates, per tree (an extension, include/mi_phylo.h), per pattern and
// unweighted: state_posteriors_ [n-2][P][4] of the internal nodes n .. 2n-3 (row v - n) and, asked
// for, map_states_ [n-2][P], category_posteriors_ [P][K] with pattern_rates_ [P], and
// tip_posteriors_ [n][P][4]; what was not asked for stays empty
struct AncestralStatePosteriors {
  double log_likelihood_ = 0.;
  std::vector<double> state_posteriors_;
  std::vector<int8_t> map_states_;
  std::vector<double> category_posteriors_, pattern_rates_, tip_posteriors_;
};

// Engine::Placement, per tree (an extension, include/mi_phylo.h) for Q queries and E = 2n-3 edges:
// edge_log_likelihoods_ [Q][E] and best_edge_ [Q], and, asked for, pendant_index_ [Q][E], lwr_
// [Q][E] and tables_ [E][G][5][P]; what was not asked for stays empty
struct PlacementResult {
  double log_likelihood_ = 0.;
  std::vector<double> edge_log_likelihoods_;
  std::vector<int32_t> best_edge_;
  std::vector<int8_t> pendant_index_;
  std::vector<double> lwr_, tables_;
};

// Engine::SprScan, per tree (an extension, include/mi_phylo.h) with E = 2n-3 edges: per (pruned
// edge s, direction) the target of the largest log-likelihood change best_target_ [E][2] (-1: no
// move) and that change best_delta_ [E][2] (-inf: no move); best_move_ = (s, direction, f) of the
// tree's largest change; asked for, delta_ [E][2][E], the whole table (-inf: no move)
struct SprNeighbourhood {
  double log_likelihood_ = 0.;
  std::vector<int32_t> best_target_;
  std::vector<double> best_delta_;
  int32_t best_move_[3] = {-1, -1, -1};
  std::vector<double> delta_;
};

// Engine::OptimizeBranchLengths, per tree (an extension, include/mi_phylo.h): the
// maximum-likelihood branch lengths [2n-2] and the Hessian call's outputs at them [2n-1]
struct BranchOptimum {
  std::vector<double> branch_lengths_;
  double log_likelihood_ = 0.;
  std::vector<double> gradient_, hessian_;
  int32_t iterations_ = 0;
  int32_t status_ = 0;  // MI_BRANCH_OPT_*
};

// Engine::NniSearch, per tree (an extension, include/mi_phylo.h): topology [2n-3] and lengths
// [2n-2] of the last optimisation, its logL, the largest NNI delta there, the codes 2 v + i (in
// the ids of the tree at that round) and deltas of the moves taken
struct NniSearchEnd {
  std::vector<int32_t> parent_ids_;
  std::vector<double> branch_lengths_;
  double log_likelihood_ = 0., best_delta_ = 0.;
  std::vector<int32_t> moves_;
  std::vector<double> gains_;
  int32_t status_ = 0;             // MI_NNI_SEARCH_*
  int32_t branch_opt_status_ = 0;  // MI_BRANCH_OPT_*
};

// Engine::SprSearch, per tree (an extension, include/mi_phylo.h): as NniSearchEnd, with the
// triples (s, dir, f) of the moves taken, three entries of moves_ per move
struct SprSearchEnd {
  std::vector<int32_t> parent_ids_;
  std::vector<double> branch_lengths_;
  double log_likelihood_ = 0., best_delta_ = 0.;
  std::vector<int32_t> moves_;
  std::vector<double> gains_;
  int32_t status_ = 0;             // MI_SPR_SEARCH_*
  int32_t branch_opt_status_ = 0;  // MI_BRANCH_OPT_*
};

struct ParamMatrix {  // row-major [rows x cols]
  size_t rows = 0, cols = 0;
  std::vector<double> data;
  ParamMatrix() = default;
  ParamMatrix(size_t r, size_t c) : rows(r), cols(c), data(r * c, 0.) {}
  double& operator()(size_t r, size_t c) { return data[r * cols + c]; }
  void SetBlock(size_t start, size_t length, const std::vector<double>& values) {
    for (size_t r = 0; r < rows; r++)
      for (size_t i = 0; i < length; i++) data[r * cols + start + i] = values[i % values.size()];
  }
};

using UnrootedTreeCollection = std::vector<FlatTree>;
using RootedTreeCollection = std::vector<RootedFlatTree>;
using BlockSpecificationMap = std::map<std::string, std::pair<size_t, size_t>>;

class Engine {
 public:
  Engine(const EngineSpecification& engine_specification,
         const PhyloModelSpecification& specification, SitePattern site_pattern)
      : site_pattern_(std::move(site_pattern)) {
    if (engine_specification.thread_count_ == 0)
      Failwith("Thread count needs to be strictly positive.");
    mi_engine_spec spec{};
    spec.taxon_count = static_cast<int32_t>(site_pattern_.SequenceCount());
    spec.pattern_count = static_cast<int32_t>(site_pattern_.PatternCount());
    spec.state_count = 4;
    if (specification.substitution_ == "JC69") spec.subst_model = MI_SUBST_JC69;
    else if (specification.substitution_ == "GTR") spec.subst_model = MI_SUBST_GTR;
    else if (specification.substitution_ == "WAG") {  // 20 states, built-in table
      spec.subst_model = MI_SUBST_REVERSIBLE;
      spec.state_count = 20;
    } else Failwith("Substitution model not known: " + specification.substitution_);
    if (site_pattern_.StateCount() != spec.state_count)
      Failwith("The site pattern is coded in a " + std::to_string(site_pattern_.StateCount()) +
               "-state alphabet, the substitution model " + specification.substitution_ +
               " has " + std::to_string(spec.state_count) + " states.");
    if (specification.site_ == "constant") {
      spec.site_model = MI_SITE_CONSTANT;
      spec.category_count = 1;
    } else if (specification.site_.rfind("weibull", 0) == 0) {  // site_model.cpp:15-22
      spec.site_model = MI_SITE_WEIBULL;
      const auto plus = specification.site_.find("+");
      spec.category_count =
          plus == std::string::npos ? 4 : std::stoi(specification.site_.substr(plus + 1));
    } else {
      Failwith("Site model not known: " + specification.site_);
    }
    if (specification.clock_ == "none") spec.clock_model = MI_CLOCK_NONE;
    else if (specification.clock_ == "strict") spec.clock_model = MI_CLOCK_STRICT;
    else Failwith("Clock model not known: " + specification.clock_);
    spec.use_tip_states = engine_specification.use_tip_states_;
    spec.device = -1;
    category_count_ = spec.category_count;
    is_gtr_ = spec.subst_model == MI_SUBST_GTR;
    const auto tips = site_pattern_.FlatPatterns();
    std::vector<int32_t> shards = engine_specification.device_shards_;
    if (shards.empty()) {
      // thread_count executors (engine.cpp:23-27) = that many devices, counted from the
      // caller's CURRENT HIP device (ordinal -1 - i, include/mi_phylo.h): one executor stays
      // on the device the process selected -- under one-process-per-GPU launches every rank
      // would otherwise pile onto device 0
      const size_t devices = static_cast<size_t>(std::max(1, mi_device_count()));
      for (size_t i = 0; i < std::min(engine_specification.thread_count_, devices); i++)
        shards.push_back(-1 - static_cast<int32_t>(i));
    }
    taxon_count_ = static_cast<size_t>(spec.taxon_count);
    Check(mi_engine_create_sharded(&spec, static_cast<int32_t>(shards.size()), shards.data(),
                                   MI_SHARD_TREES, nullptr, nullptr, tips.data(), nullptr,
                                   site_pattern_.GetWeights().data(), &handle_));
    for (int i = 0; i < mi_engine_block_count(handle_); i++) {
      const char* name;
      int32_t start, length;
      Check(mi_engine_block(handle_, i, &name, &start, &length));
      block_specification_[name] = {static_cast<size_t>(start), static_cast<size_t>(length)};
    }
  }
  ~Engine() { mi_engine_destroy(handle_); }
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  const BlockSpecificationMap& GetPhyloModelBlockSpecification() const {
    return block_specification_;
  }
  size_t ParameterCount() const { return block_specification_.at("entire").second; }

  std::vector<double> LogLikelihoods(const UnrootedTreeCollection& trees,
                                     const ParamMatrix& params, const bool rescaling) const {
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    std::vector<double> out(trees.size());
    if (trees.empty()) return out;  // FatBeagleParallelize returns an empty vector
    Check(mi_engine_log_likelihoods_unrooted(handle_, static_cast<int32_t>(trees.size()),
                                             parents.data(), bl.data(), params.data.data(),
                                             rescaling, out.data()));
    return out;
  }

  std::vector<double> LogLikelihoods(const RootedTreeCollection& trees,
                                     const ParamMatrix& params, const bool rescaling) const {
    return RootedLogLikelihoods(trees, params, rescaling, true);
  }

  std::vector<double> UnrootedLogLikelihoods(const RootedTreeCollection& trees,
                                             const ParamMatrix& params,
                                             const bool rescaling) const {
    return RootedLogLikelihoods(trees, params, rescaling, false);
  }

  std::vector<PhyloGradient> Gradients(const UnrootedTreeCollection& trees,
                                       const ParamMatrix& params, const bool rescaling) const {
    const size_t T = trees.size(), N = 2 * site_pattern_.SequenceCount() - 1;
    // (the flat arrays are the engine's own, re-used from call to call: no allocation, no
    // zero-filling of a megabyte of outputs per call)
    std::vector<int32_t>& parents = scratch_parents_;
    std::vector<double>& bl = scratch_bl_;
    Flatten(trees, params, false, &parents, &bl);
    if (trees.empty()) return {};
    Grow(&scratch_ll_, T);
    Grow(&scratch_a_, T * N);
    Grow(&scratch_site_, T);
    Grow(&scratch_subst_, T * 8);
    const double *ll = scratch_ll_.data(), *g = scratch_a_.data(), *site = scratch_site_.data(),
                 *subst = scratch_subst_.data();
    Check(mi_engine_gradients_unrooted(handle_, static_cast<int32_t>(T), parents.data(),
                                       bl.data(), params.data.data(), rescaling, scratch_ll_.data(),
                                       scratch_a_.data(), category_count_ > 1 ? scratch_site_.data() : nullptr,
                                       is_gtr_ ? scratch_subst_.data() : nullptr));
    std::vector<PhyloGradient> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].log_likelihood_ = ll[t];
      // (keys in map order, each placed at the end with its vector built in place)
      GradientMap& m = out[t].gradient_;
      m.emplace_hint(m.end(), std::piecewise_construct, std::forward_as_tuple("branch_lengths"),
                     std::forward_as_tuple(g + t * N, g + (t + 1) * N));
      AddModelGradients(&out[t], site[t], subst + 8 * t);
    }
    return out;
  }

  // Diagonal of the branch-length Hessian per tree (an extension; 4-state engines):
  // mi_engine_branch_hessian_unrooted.  Vectors in node-id order, root and fixed node 0.
  std::vector<BranchHessian> BranchHessians(const UnrootedTreeCollection& trees,
                                            const ParamMatrix& params, const bool rescaling) const {
    const size_t T = trees.size(), N = 2 * site_pattern_.SequenceCount() - 1;
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<double> ll(T), g(T * N), h(T * N), s(T * N);
    Check(mi_engine_branch_hessian_unrooted(handle_, static_cast<int32_t>(T), parents.data(),
                                            bl.data(), params.data.data(), rescaling, ll.data(),
                                            g.data(), h.data(), s.data()));
    std::vector<BranchHessian> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].log_likelihood_ = ll[t];
      out[t].gradient_.assign(g.begin() + t * N, g.begin() + (t + 1) * N);
      out[t].hessian_.assign(h.begin() + t * N, h.begin() + (t + 1) * N);
      out[t].gradient_sq_.assign(s.begin() + t * N, s.begin() + (t + 1) * N);
    }
    return out;
  }

  // Log-likelihood change of every nearest-neighbour interchange per tree (an extension;
  // 4-state engines): mi_engine_nni_scan_unrooted.  mi_nni_neighbour builds the tree of a move.
  std::vector<NniNeighbourhood> NniScan(const UnrootedTreeCollection& trees, const ParamMatrix& params,
                                        const bool rescaling) const {
    const size_t T = trees.size(), N = 2 * site_pattern_.SequenceCount() - 1;
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<double> ll(T), d(T * N * 2);
    std::vector<int32_t> best(T);
    Check(mi_engine_nni_scan_unrooted(handle_, static_cast<int32_t>(T), parents.data(), bl.data(),
                                      params.data.data(), rescaling, ll.data(), d.data(), best.data()));
    std::vector<NniNeighbourhood> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].log_likelihood_ = ll[t];
      out[t].delta_.assign(d.begin() + t * N * 2, d.begin() + (t + 1) * N * 2);
      out[t].best_move_ = best[t];
    }
    return out;
  }

  // Log-likelihood change of every subtree-prune-and-regraft move per tree (an extension; 4-state
  // engines): mi_engine_spr_scan_unrooted.  radius 0: every move.  mi_spr_neighbour builds the
  // tree of a move.
  std::vector<SprNeighbourhood> SprScan(const UnrootedTreeCollection& trees, const ParamMatrix& params,
                                        const bool rescaling, const int32_t radius = 0,
                                        const bool table = false) const {
    const size_t T = trees.size(), E = 2 * site_pattern_.SequenceCount() - 3;
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<double> ll(T), best(T * 2 * E), d(table ? T * 2 * E * E : 0);
    std::vector<int32_t> target(T * 2 * E), move(T * 3);
    Check(mi_engine_spr_scan_unrooted(handle_, static_cast<int32_t>(T), parents.data(), bl.data(),
                                      params.data.data(), rescaling, radius, ll.data(), target.data(), best.data(),
                                      move.data(), table ? d.data() : nullptr));
    std::vector<SprNeighbourhood> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].log_likelihood_ = ll[t];
      out[t].best_target_.assign(target.begin() + t * 2 * E, target.begin() + (t + 1) * 2 * E);
      out[t].best_delta_.assign(best.begin() + t * 2 * E, best.begin() + (t + 1) * 2 * E);
      std::copy(move.begin() + t * 3, move.begin() + (t + 1) * 3, out[t].best_move_);
      if (table) out[t].delta_.assign(d.begin() + t * 2 * E * E, d.begin() + (t + 1) * 2 * E * E);
    }
    return out;
  }

  // Marginal ancestral-state posteriors per tree, internal node and pattern (an extension;
  // 4-state engines): mi_engine_ancestral_states_unrooted.
  std::vector<AncestralStatePosteriors> AncestralStates(const UnrootedTreeCollection& trees,
                                                        const ParamMatrix& params, const bool rescaling,
                                                        const bool map_states = false, const bool categories = false,
                                                        const bool tips = false) const {
    const size_t T = trees.size(), n = site_pattern_.SequenceCount(), P = site_pattern_.PatternCount();
    const size_t K = static_cast<size_t>(category_count_), rows = (n - 2) * P;
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<double> ll(T), state(T * rows * 4), cat(categories ? T * P * K : 0), rate(categories ? T * P : 0),
        tip(tips ? T * n * P * 4 : 0);
    std::vector<int8_t> map(map_states ? T * rows : 0);
    Check(mi_engine_ancestral_states_unrooted(handle_, static_cast<int32_t>(T), parents.data(), bl.data(),
                                              params.data.data(), rescaling, ll.data(), state.data(),
                                              map_states ? map.data() : nullptr, categories ? cat.data() : nullptr,
                                              categories ? rate.data() : nullptr, tips ? tip.data() : nullptr));
    std::vector<AncestralStatePosteriors> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].log_likelihood_ = ll[t];
      out[t].state_posteriors_.assign(state.begin() + t * rows * 4, state.begin() + (t + 1) * rows * 4);
      if (map_states) out[t].map_states_.assign(map.begin() + t * rows, map.begin() + (t + 1) * rows);
      if (categories) {
        out[t].category_posteriors_.assign(cat.begin() + t * P * K, cat.begin() + (t + 1) * P * K);
        out[t].pattern_rates_.assign(rate.begin() + t * P, rate.begin() + (t + 1) * P);
      }
      if (tips) out[t].tip_posteriors_.assign(tip.begin() + t * n * P * 4, tip.begin() + (t + 1) * n * P * 4);
    }
    return out;
  }

  // Phylogenetic placement (an extension; 4-state engines): mi_engine_placement_unrooted.  queries
  // [Q][C] compact states, column_pattern [C], column_weights [C] or empty (1 per column).
  std::vector<PlacementResult> Placement(const UnrootedTreeCollection& trees, const ParamMatrix& params,
                                         const bool rescaling, const std::vector<int8_t>& queries,
                                         const std::vector<int32_t>& column_pattern,
                                         const std::vector<double>& column_weights,
                                         const std::vector<double>& pendant_lengths, const bool pendant_index = false,
                                         const bool lwr = false, const bool tables = false) const {
    const size_t T = trees.size(), n = site_pattern_.SequenceCount(), P = site_pattern_.PatternCount();
    const size_t E = 2 * n - 3, C = column_pattern.size(), G = pendant_lengths.size();
    const size_t Q = C ? queries.size() / C : 0, QE = Q * E, tab = E * G * 5 * P;
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<double> ll(T), edge(T * QE), w(lwr ? T * QE : 0), tb(tables ? T * tab : 0);
    std::vector<int32_t> best(T * Q);
    std::vector<int8_t> pend(pendant_index ? T * QE : 0);
    Check(mi_engine_placement_unrooted(
        handle_, static_cast<int32_t>(T), parents.data(), bl.data(), params.data.data(), rescaling,
        static_cast<int32_t>(Q), static_cast<int32_t>(C), queries.data(), column_pattern.data(),
        column_weights.empty() ? nullptr : column_weights.data(), static_cast<int32_t>(G), pendant_lengths.data(),
        ll.data(), edge.data(), pendant_index ? pend.data() : nullptr, best.data(), lwr ? w.data() : nullptr,
        tables ? tb.data() : nullptr));
    std::vector<PlacementResult> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].log_likelihood_ = ll[t];
      out[t].edge_log_likelihoods_.assign(edge.begin() + t * QE, edge.begin() + (t + 1) * QE);
      out[t].best_edge_.assign(best.begin() + t * Q, best.begin() + (t + 1) * Q);
      if (pendant_index) out[t].pendant_index_.assign(pend.begin() + t * QE, pend.begin() + (t + 1) * QE);
      if (lwr) out[t].lwr_.assign(w.begin() + t * QE, w.begin() + (t + 1) * QE);
      if (tables) out[t].tables_.assign(tb.begin() + t * tab, tb.begin() + (t + 1) * tab);
    }
    return out;
  }

  // Unweighted per-pattern log-likelihoods log L_p per tree (an extension; 4-state engines):
  // mi_engine_pattern_log_likelihoods_unrooted.
  PatternLogLikelihood PatternLogLikelihoods(const UnrootedTreeCollection& trees, const ParamMatrix& params,
                                             const bool rescaling) const {
    const size_t T = trees.size(), P = site_pattern_.PatternCount();
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    PatternLogLikelihood out;
    if (trees.empty()) return out;
    out.log_likelihoods_.resize(T);
    out.pattern_log_likelihoods_.resize(T * P);
    Check(mi_engine_pattern_log_likelihoods_unrooted(handle_, static_cast<int32_t>(T), parents.data(), bl.data(),
                                                     params.data.data(), rescaling, out.log_likelihoods_.data(),
                                                     out.pattern_log_likelihoods_.data()));
    return out;
  }

  // RELL bootstrap of the trees from `replicates` rows of replicate weights [B][P] (an extension;
  // 4-state engines, one device): mi_engine_rell_bootstrap_unrooted.
  RellBootstrapResult RellBootstrap(const UnrootedTreeCollection& trees, const ParamMatrix& params,
                                    const bool rescaling, const size_t replicates,
                                    const std::vector<double>& replicate_weights) const {
    const size_t T = trees.size(), P = site_pattern_.PatternCount(), B = replicates;
    if (replicate_weights.size() != B * P) Failwith("RellBootstrap: replicate weights must be [replicates][patterns].");
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    RellBootstrapResult out;
    if (trees.empty()) return out;
    out.log_likelihoods_.resize(T);
    out.pattern_log_likelihoods_.resize(T * P);
    out.replicate_log_likelihoods_.resize(B * T);
    out.best_tree_.resize(B);
    out.bootstrap_proportion_.resize(T);
    out.expected_likelihood_weight_.resize(T);
    Check(mi_engine_rell_bootstrap_unrooted(
        handle_, static_cast<int32_t>(T), parents.data(), bl.data(), params.data.data(), rescaling,
        static_cast<int32_t>(B), replicate_weights.data(), out.log_likelihoods_.data(),
        out.pattern_log_likelihoods_.data(), out.replicate_log_likelihoods_.data(), out.best_tree_.data(),
        out.bootstrap_proportion_.data(), out.expected_likelihood_weight_.data()));
    return out;
  }

  // `replicates` rows of bootstrap weights drawn on the device from the engine's pattern weights,
  // `sites` draws each (0: the ordinary bootstrap, N = sum of the weights), [replicates][P] in the
  // layout RellBootstrap, PairwiseDistances and StartingTrees take (an extension):
  // mi_engine_bootstrap_weights.
  std::vector<double> BootstrapWeights(const size_t replicates, const int64_t sites, const uint64_t seed,
                                       const int64_t first_replicate) const {
    const std::vector<double>& w = site_pattern_.GetWeights();
    double total = 0.;
    for (const double x : w) total += x;
    std::vector<double> out(replicates * w.size());
    Check(mi_engine_bootstrap_weights(handle_, static_cast<int32_t>(w.size()), w.data(),
                                      static_cast<int32_t>(replicates), sites > 0 ? sites : static_cast<int64_t>(total),
                                      seed, first_replicate, out.data()));
    return out;
  }

  // The KH, SH and AU tests of the trees with BP and ELW, from trees to the table in one call (an
  // extension; 4-state engines, one device): mi_engine_topology_tests_unrooted.  Block k draws
  // replicates replicates of floor(scales[k] N + 0.5) sites; scales[0] must be 1.
  TopologyTestsResult TopologyTests(const UnrootedTreeCollection& trees, const ParamMatrix& params,
                                    const bool rescaling,
                                    const std::vector<double>& scales = {1.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.1, 1.2, 1.3, 1.4},
                                    const size_t replicates = 10000, const uint64_t seed = 0,
                                    const int64_t first_replicate = 0) const {
    const size_t T = trees.size(), P = site_pattern_.PatternCount(), K = scales.size();
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    TopologyTestsResult out;
    if (trees.empty()) return out;
    double total = 0.;
    for (const double x : site_pattern_.GetWeights()) total += x;
    out.replicates_.assign(K, static_cast<int32_t>(replicates));
    for (const double scale : scales) out.sites_.push_back(static_cast<int64_t>(std::floor(scale * total + 0.5)));
    out.log_likelihoods_.resize(T);
    out.pattern_log_likelihoods_.resize(T * P);
    out.table_.resize(T * MI_TOPOLOGY_COLUMNS);
    out.counts_.resize(K * T);
    out.column_mean_.resize(T);
    Check(mi_engine_topology_tests_unrooted(
        handle_, static_cast<int32_t>(T), parents.data(), bl.data(), params.data.data(), rescaling,
        static_cast<int32_t>(K), out.sites_.data(), out.replicates_.data(), seed, first_replicate,
        out.log_likelihoods_.data(), out.pattern_log_likelihoods_.data(), out.table_.data(), out.counts_.data(),
        out.column_mean_.data(), nullptr, nullptr));
    return out;
  }

  // Maximum-likelihood distances of all pairs of taxa for `replicates` rows of replicate weights
  // [B][P] (empty: one replicate, the engine's pattern weights) under ONE parameter row (an
  // extension; 4-state engines): mi_engine_pairwise_distances.  options == nullptr: the defaults
  // of include/mi_phylo.h.
  PairwiseDistanceResult PairwiseDistances(const size_t replicates, const std::vector<double>& replicate_weights,
                                           const std::vector<double>& param_row,
                                           const mi_distance_options* options = nullptr) const {
    const size_t n = site_pattern_.SequenceCount(), B = CheckReplicates(replicates, replicate_weights, param_row);
    PairwiseDistanceResult out;
    out.distances_.resize(B * n * n);
    out.pair_counts_.resize(B * (n * (n - 1) / 2) * 16);
    out.pair_status_.resize(B * (n * (n - 1) / 2));
    Check(mi_engine_pairwise_distances(handle_, static_cast<int32_t>(B),
                                       replicate_weights.empty() ? nullptr : replicate_weights.data(),
                                       param_row.data(), options, out.distances_.data(), out.pair_counts_.data(),
                                       out.pair_status_.data()));
    return out;
  }

  // Neighbour joining of `matrices` distance matrices [B][n][n] of `taxon_count` taxa (an
  // extension; any engine): mi_engine_neighbour_joining.  Lengths clamped into the box.
  StartingTreeResult NeighbourJoining(const size_t matrices, const size_t taxon_count,
                                      const std::vector<double>& distances, const double min_length = 1e-8,
                                      const double max_length = 10.) const {
    const size_t B = matrices, n = taxon_count;
    if (B < 1 || n < 3 || distances.size() != B * n * n)
      Failwith("NeighbourJoining: distances must be [matrices][taxa][taxa], at least three taxa.");
    StartingTreeResult out;
    out.parent_ids_.resize(B * (2 * n - 3));
    out.branch_lengths_.resize(B * (2 * n - 2));
    Check(mi_engine_neighbour_joining(handle_, static_cast<int32_t>(B), static_cast<int32_t>(n), distances.data(),
                                      min_length, max_length, out.parent_ids_.data(), out.branch_lengths_.data()));
    return out;
  }

  // The split table of a batch of unrooted trees (an extension; any engine serves: the taxon
  // count is the trees'): mi_engine_split_index.  parent_ids [T][2n-3]; branch_lengths [T][2n-2]
  // and tree_weights [T] may be empty (they enter the statistics only).
  SplitTable SplitIndex(const size_t tree_count, const size_t taxon_count, const std::vector<int32_t>& parent_ids,
                        const std::vector<double>& branch_lengths = {},
                        const std::vector<double>& tree_weights = {}) const {
    const size_t T = tree_count, n = taxon_count;
    if (T < 1 || n < 3 || parent_ids.size() != T * (2 * n - 3) ||
        (!branch_lengths.empty() && branch_lengths.size() != T * (2 * n - 2)) ||
        (!tree_weights.empty() && tree_weights.size() != T))
      Failwith("SplitIndex: parent ids must be [trees][2 taxa - 3], lengths [trees][2 taxa - 2], weights [trees].");
    const size_t cap = T * (2 * n - 3), W = (n + 31) / 32;
    SplitTable out;
    out.taxon_count_ = n;
    out.split_index_.resize(T * (2 * n - 1));
    out.bits_.resize(cap * W);
    out.first_.resize(cap);
    out.trees_.resize(cap);
    out.stats_.resize(cap * 3);
    int32_t S = 0;
    Check(mi_engine_split_index(handle_, static_cast<int32_t>(T), static_cast<int32_t>(n), parent_ids.data(),
                                branch_lengths.empty() ? nullptr : branch_lengths.data(),
                                tree_weights.empty() ? nullptr : tree_weights.data(), static_cast<int32_t>(cap),
                                out.split_index_.data(), &S, out.bits_.data(), out.first_.data(),
                                out.trees_.data(), out.stats_.data()));
    out.split_count_ = static_cast<size_t>(S);
    out.bits_.resize(out.split_count_ * W);
    out.first_.resize(out.split_count_);
    out.trees_.resize(out.split_count_);
    out.stats_.resize(out.split_count_ * 3);
    return out;
  }

  // Robinson-Foulds distances and (with branch lengths) squared branch scores between the trees
  // of a split index [T][2n-1]: mi_engine_rf_distances.
  TreeDistances RfDistances(const size_t tree_count, const size_t taxon_count,
                            const std::vector<int32_t>& split_index,
                            const std::vector<double>& branch_lengths = {}) const {
    const size_t T = tree_count, n = taxon_count;
    if (T < 1 || n < 3 || split_index.size() != T * (2 * n - 1) ||
        (!branch_lengths.empty() && branch_lengths.size() != T * (2 * n - 2)))
      Failwith("RfDistances: the split index must be [trees][2 taxa - 1], lengths [trees][2 taxa - 2].");
    TreeDistances out;
    out.rf_.resize(T * T);
    if (!branch_lengths.empty()) out.branch_score_.resize(T * T);
    Check(mi_engine_rf_distances(handle_, static_cast<int32_t>(T), static_cast<int32_t>(n), split_index.data(),
                                 branch_lengths.empty() ? nullptr : branch_lengths.data(), out.rf_.data(),
                                 branch_lengths.empty() ? nullptr : out.branch_score_.data()));
    return out;
  }

  // The subsplit support of a batch of unrooted trees and every tree's slots (an extension; any
  // engine serves): mi_engine_sbn_index.  support_tree_count 0: all trees.
  SbnSupport SbnIndex(const size_t tree_count, const size_t taxon_count, const std::vector<int32_t>& parent_ids,
                      const size_t support_tree_count = 0) const {
    const size_t T = tree_count, n = taxon_count, T0 = support_tree_count ? support_tree_count : T;
    if (T < 1 || n < 3 || T0 > T || parent_ids.size() != T * (2 * n - 3))
      Failwith("SbnIndex: parent ids must be [trees][2 taxa - 3], the support trees at most all of them.");
    const size_t E = 2 * n - 3, W = (n + 31) / 32, rcap = T0 * E, pcap = T0 * E * 6;
    SbnSupport out;
    out.taxon_count_ = n;
    out.tree_count_ = T;
    out.support_tree_count_ = T0;
    out.parent_ids_ = parent_ids;
    out.root_index_.resize(T * E);
    out.slot_index_.resize(T * E * 6);
    out.bits_.resize(rcap * W);
    out.pcsp_clades_.resize(pcap * 3);
    out.parent_range_.resize(pcap * 2);
    out.pcsp_parent_.resize(pcap);
    int32_t counts[3] = {0, 0, 0};
    Check(mi_engine_sbn_index(handle_, static_cast<int32_t>(T), static_cast<int32_t>(n), parent_ids.data(),
                              static_cast<int32_t>(T0), static_cast<int32_t>(rcap), static_cast<int32_t>(pcap),
                              out.root_index_.data(), out.slot_index_.data(), counts, out.bits_.data(),
                              out.pcsp_clades_.data(), out.parent_range_.data(), out.pcsp_parent_.data()));
    out.rootsplit_count_ = static_cast<size_t>(counts[0]);
    out.pcsp_count_ = static_cast<size_t>(counts[1]);
    out.parent_count_ = static_cast<size_t>(counts[2]);
    out.bits_.resize(out.rootsplit_count_ * W);
    out.pcsp_clades_.resize(out.pcsp_count_ * 3);
    out.parent_range_.resize(out.parent_count_ * 2);
    out.pcsp_parent_.resize(out.pcsp_count_);
    return out;
  }

  // log p of every rooting and log q of every tree of the support's batch under log_params [P],
  // normalised or not; with tree_weights [T] or expected_counts also the E-step:
  // mi_engine_sbn_log_prob.
  SbnProbabilities SbnLogProb(const SbnSupport& support, const std::vector<double>& log_params,
                              const bool normalized = false, const bool expected_counts = false,
                              const std::vector<double>& tree_weights = {}) const {
    const size_t T = support.tree_count_, E = 2 * support.taxon_count_ - 3, P = support.ParameterCount();
    if (log_params.size() != P || (!tree_weights.empty() && tree_weights.size() != T))
      Failwith("SbnLogProb: log parameters must be [rootsplits + PCSPs], weights [trees].");
    SbnProbabilities out;
    out.rooting_log_prob_.resize(T * E);
    out.log_q_.resize(T);
    if (expected_counts) out.log_expected_counts_.resize(P);
    Check(mi_engine_sbn_log_prob(
        handle_, static_cast<int32_t>(T), static_cast<int32_t>(support.taxon_count_), support.parent_ids_.data(),
        support.root_index_.data(), support.slot_index_.data(), static_cast<int32_t>(support.rootsplit_count_),
        static_cast<int32_t>(support.pcsp_count_), static_cast<int32_t>(support.parent_count_),
        support.parent_range_.data(), log_params.data(), normalized ? 1 : 0,
        tree_weights.empty() ? nullptr : tree_weights.data(), out.rooting_log_prob_.data(), out.log_q_.data(),
        expected_counts ? out.log_expected_counts_.data() : nullptr));
    return out;
  }

  // Simple-average (MI_SBN_SA) or EM (MI_SBN_EM) training on the support's own trees, which must
  // be the first of its batch: mi_engine_sbn_train.  tree_weights [support trees] may be empty.
  SbnTraining SbnTrain(const SbnSupport& support, const int32_t method, const std::vector<double>& tree_weights = {},
                       const double alpha = 0.0, const size_t max_iter = 0, const double score_epsilon = 0.0) const {
    const size_t T = support.support_tree_count_, P = support.ParameterCount();
    if (!tree_weights.empty() && tree_weights.size() != T) Failwith("SbnTrain: weights must be [support trees].");
    SbnTraining out;
    out.log_params_.resize(P);
    out.score_history_.resize(max_iter ? max_iter : 1);
    int32_t iterations = 0;
    Check(mi_engine_sbn_train(
        handle_, static_cast<int32_t>(T), static_cast<int32_t>(support.taxon_count_), support.parent_ids_.data(),
        support.root_index_.data(), support.slot_index_.data(), static_cast<int32_t>(support.rootsplit_count_),
        static_cast<int32_t>(support.pcsp_count_), static_cast<int32_t>(support.parent_count_),
        support.parent_range_.data(), tree_weights.empty() ? nullptr : tree_weights.data(), method, alpha,
        static_cast<int32_t>(max_iter), score_epsilon, out.log_params_.data(), out.score_history_.data(),
        &iterations));
    out.score_history_.resize(static_cast<size_t>(iterations));
    return out;
  }

  // The descent table [P][2] of a support: the two parent subsplits every parameter leads to
  // (>= 0 a block of parent_range_, < 0 the leaf ~value): mi_engine_sbn_descent.
  std::vector<int32_t> SbnDescent(const SbnSupport& support) const {
    std::vector<int32_t> out(support.ParameterCount() * 2);
    Check(mi_engine_sbn_descent(
        handle_, static_cast<int32_t>(support.support_tree_count_), static_cast<int32_t>(support.taxon_count_),
        support.parent_ids_.data(), support.root_index_.data(), support.slot_index_.data(),
        static_cast<int32_t>(support.rootsplit_count_), static_cast<int32_t>(support.pcsp_count_),
        support.pcsp_parent_.data(), out.data()));
    return out;
  }

  // sample_count topologies drawn from the SBN with (unnormalised) log_params [P]; sample k is the
  // Philox stream (seed, first_sample + k): mi_engine_sbn_sample.
  SbnSamples SbnSample(const SbnSupport& support, const std::vector<int32_t>& descent,
                       const std::vector<double>& log_params, const size_t sample_count, const uint64_t seed,
                       const int64_t first_sample = 0) const {
    const size_t K = sample_count, n = support.taxon_count_, P = support.ParameterCount();
    if (log_params.size() != P || descent.size() != 2 * P)
      Failwith("SbnSample: log parameters must be [rootsplits + PCSPs], the descent table twice that.");
    SbnSamples out;
    out.parent_ids_.resize(K * (2 * n - 3));
    out.root_edge_.resize(K);
    out.sampled_params_.resize(K * (n - 1));
    out.log_prob_.resize(K);
    out.cdf_.resize(P);
    Check(mi_engine_sbn_sample(
        handle_, static_cast<int32_t>(K), static_cast<int32_t>(n), static_cast<int32_t>(support.rootsplit_count_),
        static_cast<int32_t>(support.pcsp_count_), static_cast<int32_t>(support.parent_count_),
        support.parent_range_.data(), descent.data(), log_params.data(), seed, first_sample, out.parent_ids_.data(),
        out.root_edge_.data(), out.sampled_params_.data(), out.log_prob_.data(), out.cdf_.data()));
    return out;
  }

  // The gradient of the multi-sample variational objective with respect to the unnormalised
  // parameters over trees first_tree .. of the support's batch (the samples, indexed behind the
  // support trees), log_f one value per such tree, estimator MI_SBN_FACTORS_PLAIN / _VIMCO /
  // _GIVEN: mi_engine_sbn_topology_gradient.
  SbnGradient SbnTopologyGradient(const SbnSupport& support, const std::vector<double>& log_params,
                                  const std::vector<double>& log_f, const int32_t estimator = MI_SBN_FACTORS_VIMCO,
                                  const size_t first_tree = 0, const bool normalized = false) const {
    const size_t E = 2 * support.taxon_count_ - 3, P = support.ParameterCount();
    if (first_tree >= support.tree_count_ || log_f.size() != support.tree_count_ - first_tree || log_params.size() != P)
      Failwith("SbnTopologyGradient: log_f must be [trees from first_tree on], log parameters [rootsplits + PCSPs].");
    const size_t K = log_f.size();
    SbnGradient out;
    out.gradient_.resize(P);
    out.factors_.resize(K);
    out.log_q_.resize(K);
    Check(mi_engine_sbn_topology_gradient(
        handle_, static_cast<int32_t>(K), static_cast<int32_t>(support.taxon_count_),
        support.parent_ids_.data() + first_tree * E, support.root_index_.data() + first_tree * E,
        support.slot_index_.data() + first_tree * E * 6, static_cast<int32_t>(support.rootsplit_count_),
        static_cast<int32_t>(support.pcsp_count_), static_cast<int32_t>(support.parent_count_),
        support.parent_range_.data(), log_params.data(), normalized ? 1 : 0, log_f.data(), estimator,
        out.gradient_.data(), out.factors_.data(), out.log_q_.data()));
    return out;
  }

  // The PSP numbering of a support: mi_engine_psp_table.
  PspNumbering PspTable(const SbnSupport& support) const {
    PspNumbering out;
    out.psp_of_pcsp_.resize(support.pcsp_count_);
    int32_t counts[2] = {0, 0};
    Check(mi_engine_psp_table(handle_, static_cast<int32_t>(support.rootsplit_count_),
                              static_cast<int32_t>(support.pcsp_count_), support.pcsp_clades_.data(),
                              out.psp_of_pcsp_.data(), counts));
    out.rootsplit_count_ = static_cast<size_t>(counts[0]);
    out.variable_count_ = static_cast<size_t>(counts[1]);
    return out;
  }

  // The index rows [trees from first_tree on][rows][2n-3] of a support's batch, rows 1 (splits) or
  // 3 (split, down PSP, up PSP): mi_engine_psp_index.
  std::vector<int32_t> PspIndex(const SbnSupport& support, const PspNumbering& table, const size_t rows = 3,
                                const size_t first_tree = 0) const {
    const size_t E = 2 * support.taxon_count_ - 3;
    if (first_tree >= support.tree_count_ || table.psp_of_pcsp_.size() != support.pcsp_count_)
      Failwith("PspIndex: the table must be the support's, first_tree one of its trees.");
    const size_t T = support.tree_count_ - first_tree;
    std::vector<int32_t> out(T * rows * E);
    Check(mi_engine_psp_index(handle_, static_cast<int32_t>(T), static_cast<int32_t>(support.taxon_count_),
                              support.root_index_.data() + first_tree * E,
                              support.slot_index_.data() + first_tree * E * 6,
                              static_cast<int32_t>(support.rootsplit_count_), static_cast<int32_t>(support.pcsp_count_),
                              table.psp_of_pcsp_.data(), static_cast<int32_t>(table.variable_count_),
                              static_cast<int32_t>(rows), out.data()));
    return out;
  }

  // Branch lengths of tree_count particles from the log-normal q with q_params [V][2] summed over
  // index [T][rows][2n-3]; particle t is the Philox stream (seed, first_sample + t), or takes
  // epsilon [T][2n-3] if given: mi_engine_branch_model_sample.
  BranchModelDraw BranchModelSample(const size_t tree_count, const size_t taxon_count, const size_t rows,
                                    const std::vector<int32_t>& index, const std::vector<double>& q_params,
                                    const uint64_t seed, const int64_t first_sample = 0, const double prior_rate = 10.0,
                                    const std::vector<double>& epsilon = {}) const {
    const size_t T = tree_count, E = 2 * taxon_count - 3;
    if (index.size() != T * rows * E || q_params.size() % 2 || (!epsilon.empty() && epsilon.size() != T * E))
      Failwith("BranchModelSample: index must be [trees][rows][2 taxa - 3], q_params [V][2], epsilon [trees][2 taxa - 3].");
    BranchModelDraw out;
    out.branch_lengths_.resize(T * (E + 1));
    out.epsilon_.resize(T * E);
    out.log_q_.resize(T);
    out.log_prior_.resize(T);
    Check(mi_engine_branch_model_sample(
        handle_, static_cast<int32_t>(T), static_cast<int32_t>(taxon_count), static_cast<int32_t>(rows), index.data(),
        static_cast<int32_t>(q_params.size() / 2), q_params.data(), seed, first_sample, prior_rate,
        epsilon.empty() ? nullptr : epsilon.data(), out.branch_lengths_.data(), out.epsilon_.data(), out.log_q_.data(),
        out.log_prior_.data()));
    return out;
  }

  // The gradient with respect to q_params and log_f for a draw of the same index and q_params,
  // from the likelihood call's branch gradients [T][2n-1] and log-likelihoods [T];
  // log_q_topology and tree_weights may be empty: mi_engine_branch_model_gradient.
  BranchModelGradientResult BranchModelGradient(const size_t tree_count, const size_t taxon_count, const size_t rows,
                                                const std::vector<int32_t>& index, const std::vector<double>& q_params,
                                                const BranchModelDraw& draw, const std::vector<double>& branch_gradient,
                                                const std::vector<double>& log_likelihoods,
                                                const std::vector<double>& log_q_topology = {},
                                                const std::vector<double>& tree_weights = {}, const double beta = 1.0,
                                                const double prior_rate = 10.0) const {
    const size_t T = tree_count, E = 2 * taxon_count - 3;
    if (index.size() != T * rows * E || q_params.size() % 2 || draw.epsilon_.size() != T * E ||
        branch_gradient.size() != T * (E + 2) || log_likelihoods.size() != T ||
        (!log_q_topology.empty() && log_q_topology.size() != T) || (!tree_weights.empty() && tree_weights.size() != T))
      Failwith("BranchModelGradient: the arrays must be those of one batch of trees.");
    BranchModelGradientResult out;
    out.gradient_.resize(q_params.size());
    out.log_f_.resize(T);
    Check(mi_engine_branch_model_gradient(
        handle_, static_cast<int32_t>(T), static_cast<int32_t>(taxon_count), static_cast<int32_t>(rows), index.data(),
        static_cast<int32_t>(q_params.size() / 2), q_params.data(), draw.branch_lengths_.data(), draw.epsilon_.data(),
        draw.log_q_.data(), draw.log_prior_.data(), branch_gradient.data(), log_likelihoods.data(),
        log_q_topology.empty() ? nullptr : log_q_topology.data(), tree_weights.empty() ? nullptr : tree_weights.data(),
        beta, prior_rate, out.gradient_.data(), out.log_f_.data()));
    return out;
  }

  // A device-resident variational fit over the support of support_parent_ids [T0][2n-3] on this
  // engine's alignment, from log_params [P] and q_params [V][2]; options as
  // mi_vi_default_options leaves them unless given; model_param_row: the one row every particle
  // takes: mi_engine_vi_create.
  static mi_vi_options ViDefaultOptions() {
    mi_vi_options o;
    Check(mi_vi_default_options(&o));
    return o;
  }
  VariationalFit ViCreate(const size_t support_tree_count, const std::vector<int32_t>& support_parent_ids,
                          const std::vector<double>& log_params, const std::vector<double>& q_params,
                          const mi_vi_options& options, const std::vector<double>& model_param_row = {}) const {
    if (support_parent_ids.size() != support_tree_count * (2 * taxon_count_ - 3) || q_params.size() % 2)
      Failwith("ViCreate: the support is [trees][2n-3] on the engine's taxa, q_params [V][2].");
    if (!model_param_row.empty() && model_param_row.size() != static_cast<size_t>(ParameterCount()))
      Failwith("ViCreate takes ONE parameter row.");
    mi_vi* handle = nullptr;
    Check(mi_engine_vi_create(handle_, static_cast<int32_t>(support_tree_count),
                              support_tree_count ? support_parent_ids.data() : nullptr,
                              model_param_row.empty() ? nullptr : model_param_row.data(),
                              static_cast<int32_t>(log_params.size()), log_params.data(),
                              static_cast<int32_t>(q_params.size() / 2), q_params.data(), &options, &handle));
    return VariationalFit(handle);
  }

  // Generalized pruning over the subsplit DAG of rooted topologies parent_ids [T][2n-2] on this
  // engine's alignment; branch_lengths [T][2n-1] or empty (0.1 everywhere); model_param_row: the
  // one parameter row; rescaling_threshold 0: the default: mi_engine_gp_create.
  GeneralizedPruning GpCreate(const size_t tree_count, const std::vector<int32_t>& parent_ids,
                              const std::vector<double>& branch_lengths = {},
                              const std::vector<double>& model_param_row = {},
                              const double rescaling_threshold = 0.0) const {
    if (parent_ids.size() != tree_count * (2 * taxon_count_ - 2) ||
        (!branch_lengths.empty() && branch_lengths.size() != tree_count * (2 * taxon_count_ - 1)))
      Failwith("GpCreate: parent_ids is [trees][2n-2] on the engine's taxa, branch_lengths [trees][2n-1] or empty.");
    if (!model_param_row.empty() && model_param_row.size() != static_cast<size_t>(ParameterCount()))
      Failwith("GpCreate takes ONE parameter row.");
    mi_gp* handle = nullptr;
    Check(mi_engine_gp_create(handle_, static_cast<int32_t>(tree_count), static_cast<int32_t>(taxon_count_),
                              parent_ids.data(), branch_lengths.empty() ? nullptr : branch_lengths.data(),
                              model_param_row.empty() ? nullptr : model_param_row.data(), rescaling_threshold, &handle));
    return GeneralizedPruning(handle);
  }

  // A DAG-only GeneralizedPruning on any engine (mi_engine_gp_create_dag): the DAG, numbering, initial
  // q and b of GpCreate, no vectors; it serves the structure, b / q and tree calls.
  GeneralizedPruning GpCreateDag(const size_t tree_count, const std::vector<int32_t>& parent_ids,
                                 const std::vector<double>& branch_lengths = {}) const {
    if (parent_ids.size() != tree_count * (2 * taxon_count_ - 2) ||
        (!branch_lengths.empty() && branch_lengths.size() != tree_count * (2 * taxon_count_ - 1)))
      Failwith("GpCreateDag: parent_ids is [trees][2n-2] on the engine's taxa, branch_lengths [trees][2n-1] or empty.");
    mi_gp* handle = nullptr;
    Check(mi_engine_gp_create_dag(handle_, static_cast<int32_t>(tree_count), static_cast<int32_t>(taxon_count_),
                                  parent_ids.data(), branch_lengths.empty() ? nullptr : branch_lengths.data(), &handle));
    return GeneralizedPruning(handle);
  }

  // Rooted trees parent_ids [T][2n-2] of taxon_count taxa (root 2n-2; branch_lengths [T][2n-1] or empty),
  // de-rooted as Node::Deroot does and renumbered in the unrooted convention: mi_engine_deroot_trees.
  DerootedTrees DerootTrees(const size_t tree_count, const size_t taxon_count, const std::vector<int32_t>& parent_ids,
                            const std::vector<double>& branch_lengths = {}) const {
    if (parent_ids.size() != tree_count * (2 * taxon_count - 2) ||
        (!branch_lengths.empty() && branch_lengths.size() != tree_count * (2 * taxon_count - 1)))
      Failwith("DerootTrees: parent_ids is [trees][2n-2], branch_lengths [trees][2n-1] or empty.");
    DerootedTrees out;
    out.parent_ids_.resize(tree_count * (2 * taxon_count - 3));
    out.root_edge_.resize(tree_count);
    if (!branch_lengths.empty()) out.branch_lengths_.resize(tree_count * (2 * taxon_count - 2));
    Check(mi_engine_deroot_trees(handle_, static_cast<int32_t>(tree_count), static_cast<int32_t>(taxon_count), parent_ids.data(),
                                 branch_lengths.empty() ? nullptr : branch_lengths.data(), out.parent_ids_.data(),
                                 branch_lengths.empty() ? nullptr : out.branch_lengths_.data(), out.root_edge_.data()));
    return out;
  }

  // `steps` steps of a fit; their trace rows [steps][6]: mi_vi_fit.
  std::vector<double> ViFit(const VariationalFit& fit, const size_t steps, const int check_interval = 0) const {
    std::vector<double> trace(6 * steps);
    Check(mi_vi_fit(fit.Handle(), static_cast<int32_t>(steps), check_interval, trace.data()));
    return trace;
  }

  // One update of a fit's state from given gradients [P], [V][2] and the particles' terms [K]
  // each; the trace row: mi_vi_update.
  std::array<double, 6> ViUpdate(const VariationalFit& fit, const std::vector<double>& sbn_gradient,
                                 const std::vector<double>& q_gradient, const std::vector<double>& log_likelihoods,
                                 const std::vector<double>& log_prior, const std::vector<double>& log_q_topology,
                                 const std::vector<double>& log_q_branch) const {
    const auto sizes = fit.Sizes();
    const size_t K = sizes[1], V = sizes[6], P = sizes[8];
    if (sbn_gradient.size() != P || q_gradient.size() != 2 * V || log_likelihoods.size() != K ||
        log_prior.size() != K || log_q_topology.size() != K || log_q_branch.size() != K)
      Failwith("ViUpdate: gradients [P] and [V][2], the particles' terms [K] each.");
    std::array<double, 6> row{};
    Check(mi_vi_update(fit.Handle(), sbn_gradient.data(), q_gradient.data(), log_likelihoods.data(), log_prior.data(),
                       log_q_topology.data(), log_q_branch.data(), row.data()));
    return row;
  }

  // The whole state of a fit: mi_vi_get_state.
  ViStateResult ViState(const VariationalFit& fit) const {
    const auto sizes = fit.Sizes();
    const size_t V = sizes[6], P = sizes[8];
    ViStateResult out;
    out.log_params_.resize(P);
    out.q_params_.resize(2 * V);
    out.sbn_moments_.resize(2 * P);
    out.q_moments_.resize(4 * V);
    Check(mi_vi_get_state(fit.Handle(), out.log_params_.data(), out.q_params_.data(), out.sbn_moments_.data(),
                          out.q_moments_.data(), out.scalars_.data(), out.counters_.data()));
    return out;
  }

  // PairwiseDistances followed by NeighbourJoining in one call, nothing returning to the host in
  // between (an extension; 4-state engines): mi_engine_starting_trees_unrooted.
  StartingTreeResult StartingTrees(const size_t replicates, const std::vector<double>& replicate_weights,
                                   const std::vector<double>& param_row,
                                   const mi_distance_options* options = nullptr) const {
    const size_t n = site_pattern_.SequenceCount(), B = CheckReplicates(replicates, replicate_weights, param_row);
    StartingTreeResult out;
    out.parent_ids_.resize(B * (2 * n - 3));
    out.branch_lengths_.resize(B * (2 * n - 2));
    out.distances_.resize(B * n * n);
    Check(mi_engine_starting_trees_unrooted(handle_, static_cast<int32_t>(B),
                                            replicate_weights.empty() ? nullptr : replicate_weights.data(),
                                            param_row.data(), options, out.parent_ids_.data(),
                                            out.branch_lengths_.data(), out.distances_.data()));
    return out;
  }

  // Maximum-likelihood branch lengths per tree, started from the trees' own lengths
  // (an extension; 4-state engines): mi_engine_optimize_branch_lengths_unrooted.
  // options == nullptr: the defaults of include/mi_phylo.h.
  std::vector<BranchOptimum> OptimizeBranchLengths(const UnrootedTreeCollection& trees,
                                                   const ParamMatrix& params, const bool rescaling,
                                                   const mi_branch_opt_options* options = nullptr) const {
    const size_t T = trees.size(), N = 2 * site_pattern_.SequenceCount() - 1;
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<double> t(T * (N - 1)), ll(T), g(T * N), h(T * N);
    std::vector<int32_t> iters(T), status(T);
    Check(mi_engine_optimize_branch_lengths_unrooted(
        handle_, static_cast<int32_t>(T), parents.data(), bl.data(), params.data.data(), rescaling,
        options, t.data(), ll.data(), g.data(), h.data(), iters.data(), status.data()));
    std::vector<BranchOptimum> out(T);
    for (size_t i = 0; i < T; i++) {
      out[i].branch_lengths_.assign(t.begin() + i * (N - 1), t.begin() + (i + 1) * (N - 1));
      out[i].log_likelihood_ = ll[i];
      out[i].gradient_.assign(g.begin() + i * N, g.begin() + (i + 1) * N);
      out[i].hessian_.assign(h.begin() + i * N, h.begin() + (i + 1) * N);
      out[i].iterations_ = iters[i];
      out[i].status_ = status[i];
    }
    return out;
  }

  // One NNI move per tree on the device (an extension): mi_engine_nni_apply_unrooted.  moves[t]
  // = 2 v + i as NniScan's best_move_ gives it, or -1: the tree as it is.  Returns per tree
  // (parent ids [2n-3], branch lengths [2n-2]) in the reference's numbering.
  std::vector<std::pair<std::vector<int32_t>, std::vector<double>>> NniApply(
      const UnrootedTreeCollection& trees, const std::vector<int32_t>& moves) const {
    const size_t T = trees.size(), N = 2 * site_pattern_.SequenceCount() - 1;
    if (moves.size() != T) Failwith("NniApply needs one move per tree.");
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, ParamMatrix(T, ParameterCount()), false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<int32_t> out_pid(T * (N - 2));
    std::vector<double> out_bl(T * (N - 1));
    Check(mi_engine_nni_apply_unrooted(handle_, static_cast<int32_t>(T), parents.data(), bl.data(),
                                       moves.data(), out_pid.data(), out_bl.data()));
    std::vector<std::pair<std::vector<int32_t>, std::vector<double>>> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].first.assign(out_pid.begin() + t * (N - 2), out_pid.begin() + (t + 1) * (N - 2));
      out[t].second.assign(out_bl.begin() + t * (N - 1), out_bl.begin() + (t + 1) * (N - 1));
    }
    return out;
  }

  // NNI hill climbing per tree, started from the trees' own lengths (an extension; 4-state
  // engines): mi_engine_nni_search_unrooted.  options == nullptr: the defaults of
  // include/mi_phylo.h.
  std::vector<NniSearchEnd> NniSearch(const UnrootedTreeCollection& trees, const ParamMatrix& params,
                                      const bool rescaling,
                                      const mi_nni_search_options* options = nullptr) const {
    return Search<NniSearchEnd>(mi_engine_nni_search_unrooted, 1, trees, params, rescaling, options);
  }

  // One SPR move per tree on the device (an extension): mi_engine_spr_apply_unrooted.  moves
  // holds a triple (s, dir, f) per tree as the SPR scan's best move gives it, or (-1, -1, -1): the
  // tree as it is.  Returns per tree (parent ids [2n-3], branch lengths [2n-2]) in the reference's
  // numbering.
  std::vector<std::pair<std::vector<int32_t>, std::vector<double>>> SprApply(
      const UnrootedTreeCollection& trees, const std::vector<int32_t>& moves) const {
    const size_t T = trees.size(), N = 2 * site_pattern_.SequenceCount() - 1;
    if (moves.size() != 3 * T) Failwith("SprApply needs one triple (s, dir, f) per tree.");
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, ParamMatrix(T, ParameterCount()), false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<int32_t> out_pid(T * (N - 2));
    std::vector<double> out_bl(T * (N - 1));
    Check(mi_engine_spr_apply_unrooted(handle_, static_cast<int32_t>(T), parents.data(), bl.data(),
                                       moves.data(), out_pid.data(), out_bl.data()));
    std::vector<std::pair<std::vector<int32_t>, std::vector<double>>> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].first.assign(out_pid.begin() + t * (N - 2), out_pid.begin() + (t + 1) * (N - 2));
      out[t].second.assign(out_bl.begin() + t * (N - 1), out_bl.begin() + (t + 1) * (N - 1));
    }
    return out;
  }

  // SPR hill climbing per tree, started from the trees' own lengths (an extension; 4-state
  // engines): mi_engine_spr_search_unrooted.  options == nullptr: the defaults of
  // include/mi_phylo.h.
  std::vector<SprSearchEnd> SprSearch(const UnrootedTreeCollection& trees, const ParamMatrix& params,
                                      const bool rescaling,
                                      const mi_spr_search_options* options = nullptr) const {
    return Search<SprSearchEnd>(mi_engine_spr_search_unrooted, 3, trees, params, rescaling, options);
  }

  std::vector<PhyloGradient> Gradients(const RootedTreeCollection& trees,
                                       const ParamMatrix& params, const bool rescaling) const {
    const size_t T = trees.size(), n = site_pattern_.SequenceCount(), N = 2 * n - 1;
    std::vector<int32_t> parents, rate_counts;
    std::vector<double> bl, rates, heights, bounds, ratios;
    Flatten(trees, params, true, &parents, &bl);
    if (trees.empty()) return {};
    for (const auto& tree : trees) {
      if (!tree.TimeTreeHasBeenInitialized())  // rooted_tree.hpp:50-53
        Failwith("Attempted access of a time tree member that requires the time tree to be "
                 "initialized. Have you set dates for your time trees, and initialized the "
                 "time trees?");
      rates.insert(rates.end(), tree.rates_.begin(), tree.rates_.end());
      rate_counts.push_back(static_cast<int32_t>(tree.rate_count_));
      heights.insert(heights.end(), tree.node_heights_.begin(), tree.node_heights_.end());
      bounds.insert(bounds.end(), tree.node_bounds_.begin(), tree.node_bounds_.end());
      ratios.insert(ratios.end(), tree.height_ratios_.begin(), tree.height_ratios_.end());
    }
    std::vector<double> ll(T), gr(T * (n - 1)), gc(T * (N - 1)), site(T), subst(T * 8);
    Check(mi_engine_gradients_rooted(handle_, static_cast<int32_t>(T), parents.data(), bl.data(),
                                     params.data.data(), rates.data(), rate_counts.data(),
                                     heights.data(), bounds.data(), ratios.data(), rescaling,
                                     ll.data(), gr.data(), gc.data(), site.data(),
                                     subst.data()));
    std::vector<PhyloGradient> out(T);
    for (size_t t = 0; t < T; t++) {
      out[t].log_likelihood_ = ll[t];
      out[t].gradient_["ratios_root_height"].assign(gr.begin() + t * (n - 1),
                                                    gr.begin() + (t + 1) * (n - 1));
      const size_t clock_len = trees[t].rate_count_ == 1 ? 1 : N - 1;
      out[t].gradient_["clock_model"].assign(gc.begin() + t * (N - 1),
                                             gc.begin() + t * (N - 1) + clock_len);
      AddModelGradients(&out[t], site[t], &subst[8 * t]);
    }
    return out;
  }

 private:
  SitePattern site_pattern_;
  mi_engine* handle_ = nullptr;
  BlockSpecificationMap block_specification_;
  int category_count_ = 1;
  bool is_gtr_ = false;
  size_t taxon_count_ = 0;
  // flat arrays of the last call (an Engine is not used from two threads at once: neither is
  // the C handle behind it)
  mutable std::vector<int32_t> scratch_parents_;
  mutable std::vector<double> scratch_bl_, scratch_ll_, scratch_a_, scratch_site_, scratch_subst_;

  // the replicate count of a starting-tree call (empty weights: one replicate, the engine's own)
  size_t CheckReplicates(const size_t replicates, const std::vector<double>& replicate_weights,
                         const std::vector<double>& param_row) const {
    const size_t P = site_pattern_.PatternCount(), B = replicate_weights.empty() ? 1 : replicates;
    if (B < 1 || (!replicate_weights.empty() && replicate_weights.size() != B * P))
      Failwith("replicate weights must be [replicates][patterns], at least one replicate.");
    if (param_row.size() != static_cast<size_t>(ParameterCount()))
      Failwith("pairwise distances take ONE parameter row.");
    return B;
  }

  static void Check(int rc) {
    if (rc != 0) Failwith(mi_last_error());
  }

  template <class TColl>
  void Flatten(const TColl& trees, const ParamMatrix& params, bool rooted,
               std::vector<int32_t>* parents, std::vector<double>* bl) const {
    if (trees.size() != params.rows)  // fat_beagle.hpp:138
      Failwith("We param_matrix needs as many rows as we have trees.");
    if (params.cols != ParameterCount()) Failwith("Parameters are the wrong dimension!");
    // every tree must be on the alignment's taxa: the C ABI reads fixed-size rows
    const size_t n = taxon_count_;
    const size_t want_parents = rooted ? 2 * n - 2 : 2 * n - 3, want_bl = want_parents + 1;
    for (const auto& tree : trees)
      if (tree.parent_ids.size() != want_parents || tree.branch_lengths.size() != want_bl)
        Failwith("Tree does not have the taxon count of the site pattern (expected " +
                 std::to_string(want_parents) + " parent ids and " + std::to_string(want_bl) +
                 " branch lengths).");
    parents->resize(trees.size() * want_parents);
    bl->resize(trees.size() * want_bl);
    int32_t* pp = parents->data();
    double* pb = bl->data();
    for (const auto& tree : trees) {
      pp = std::copy(tree.parent_ids.begin(), tree.parent_ids.end(), pp);
      pb = std::copy(tree.branch_lengths.begin(), tree.branch_lengths.end(), pb);
    }
  }

  // NniSearch and SprSearch: the C function of the kind of move, the entries of moves_ per move
  template <class End, class Fn, class Options>
  std::vector<End> Search(Fn search, const size_t width, const UnrootedTreeCollection& trees,
                          const ParamMatrix& params, const bool rescaling, const Options* options) const {
    const size_t T = trees.size(), N = 2 * site_pattern_.SequenceCount() - 1;
    const size_t M = options ? static_cast<size_t>(std::max(options->max_moves, 0)) : 100;
    std::vector<int32_t> parents;
    std::vector<double> bl;
    Flatten(trees, params, false, &parents, &bl);
    if (trees.empty()) return {};
    std::vector<int32_t> pid(T * (N - 2)), count(T), log(width * T * M + 1), status(T), opt_status(T);
    std::vector<double> t(T * (N - 1)), ll(T), delta(T), gain(T * M + 1);
    Check(search(handle_, static_cast<int32_t>(T), parents.data(), bl.data(), params.data.data(), rescaling,
                 options, pid.data(), t.data(), ll.data(), delta.data(), count.data(), log.data(), gain.data(),
                 status.data(), opt_status.data()));
    std::vector<End> out(T);
    for (size_t i = 0; i < T; i++) {
      out[i].parent_ids_.assign(pid.begin() + i * (N - 2), pid.begin() + (i + 1) * (N - 2));
      out[i].branch_lengths_.assign(t.begin() + i * (N - 1), t.begin() + (i + 1) * (N - 1));
      out[i].log_likelihood_ = ll[i];
      out[i].best_delta_ = delta[i];
      out[i].moves_.assign(log.begin() + width * i * M, log.begin() + width * (i * M + count[i]));
      out[i].gains_.assign(gain.begin() + i * M, gain.begin() + i * M + count[i]);
      out[i].status_ = status[i];
      out[i].branch_opt_status_ = opt_status[i];
    }
    return out;
  }

  std::vector<double> RootedLogLikelihoods(const RootedTreeCollection& trees,
                                           const ParamMatrix& params, bool rescaling,
                                           bool with_jacobian) const {
    std::vector<int32_t> parents;
    std::vector<double> bl, rates, heights, bounds;
    Flatten(trees, params, true, &parents, &bl);
    if (trees.empty()) return {};
    if (with_jacobian)
      for (const auto& tree : trees) {
        if (!tree.TimeTreeHasBeenInitialized())
          Failwith("Attempted access of a time tree member that requires the time tree to be "
                   "initialized. Have you set dates for your time trees, and initialized the "
                   "time trees?");
        rates.insert(rates.end(), tree.rates_.begin(), tree.rates_.end());
        heights.insert(heights.end(), tree.node_heights_.begin(), tree.node_heights_.end());
        bounds.insert(bounds.end(), tree.node_bounds_.begin(), tree.node_bounds_.end());
      }
    std::vector<double> out(trees.size());
    Check(mi_engine_log_likelihoods_rooted(
        handle_, static_cast<int32_t>(trees.size()), parents.data(), bl.data(),
        params.data.data(), with_jacobian ? rates.data() : nullptr,
        with_jacobian ? heights.data() : nullptr, with_jacobian ? bounds.data() : nullptr,
        with_jacobian, rescaling, out.data()));
    return out;
  }

  // ("site_model" < "substitution_model", both after the other keys: hinted at the end)
  void AddModelGradients(PhyloGradient* g, double site, const double* subst) const {
    GradientMap& m = g->gradient_;
    if (category_count_ > 1)
      m.emplace_hint(m.end(), std::piecewise_construct, std::forward_as_tuple("site_model"),
                     std::forward_as_tuple(size_t{1}, site));
    if (is_gtr_)
      m.emplace_hint(m.end(), std::piecewise_construct, std::forward_as_tuple("substitution_model"),
                     std::forward_as_tuple(subst, subst + 8));
  }
  static void Grow(std::vector<double>* v, size_t count) {
    if (v->size() < count) v->resize(count);
  }
};

// The majority-rule consensus tree of a split table (host arithmetic only): mi_consensus_tree.
inline ConsensusTreeResult ConsensusTree(const size_t taxon_count, const std::vector<uint32_t>& split_bits,
                                         const std::vector<double>& split_weight, const double total_weight,
                                         const double threshold = 0.5) {
  const size_t n = taxon_count, W = (n + 31) / 32;
  if (n < 3 || split_bits.size() != split_weight.size() * W)
    Failwith("ConsensusTree: split bits must be [splits][ceil(taxa / 32)], weights [splits].");
  ConsensusTreeResult out;
  out.parent_ids_.resize(2 * n - 3);
  out.node_split_.resize(2 * n - 2);
  int32_t m = 0;
  if (mi_consensus_tree(static_cast<int32_t>(n), static_cast<int32_t>(split_weight.size()), split_bits.data(),
                        split_weight.data(), total_weight, threshold, &m, out.parent_ids_.data(),
                        out.node_split_.data()) != 0)
    Failwith(mi_last_error());
  out.parent_ids_.resize(static_cast<size_t>(m) - 1);
  out.node_split_.resize(static_cast<size_t>(m));
  return out;
}

}  // namespace mihost
