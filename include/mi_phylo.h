/* mi_phylo.h -- C ABI of the MI355X-native phylogenetic likelihood + gradient
 * engine.  This is the drop-in boundary for libsbn's Engine / FatBeagle path:
 * plain pointers and sizes, no C++ or torch types.
 *
 * What it replaces in the reference (paths relative to the libsbn repo root):
 *   Engine::Engine / FatBeagle::FatBeagle / CreateInstance / SetTipStates /
 *   SetTipPartials                     src/engine.cpp:10-46, src/fat_beagle.cpp:13-29,207-271
 *   Engine::LogLikelihoods (unrooted)  src/engine.cpp:54-60  -> fat_beagle.cpp:72-76
 *   Engine::LogLikelihoods (rooted)    src/engine.cpp:62-68  -> fat_beagle.cpp:96-104
 *   Engine::UnrootedLogLikelihoods     src/engine.cpp:70-76  -> fat_beagle.cpp:78-80
 *   Engine::Gradients (unrooted)       src/engine.cpp:78-84  -> fat_beagle.cpp:467-503
 *   Engine::Gradients (rooted)         src/engine.cpp:86-92  -> fat_beagle.cpp:505-545
 *   Engine::GetPhyloModelBlockSpecification  src/engine.cpp:48-52
 * together with everything those call: the 16 BEAGLE C-API calls
 * (SURVEY.md section 2.1), PhyloModel::SetParameters (src/phylo_model.cpp:26-31),
 * the GTR/JC69/Weibull models, Detrifurcate, SlideRootPosition, the rooted
 * chain rule (src/rooted_gradient_transforms.cpp) and the finite-difference
 * substitution gradient (src/fat_beagle.cpp:400-465).
 *
 * Conventions
 *   n = taxon_count, N = 2n-1, P = pattern_count, s = state_count, K = category_count.
 *   Trees arrive as the reference's own flat topology form, the parent-id vector
 *   (Node::ParentIdVector, src/node.hpp:153): leaves 0..n-1, internal nodes in
 *   post-order, root last and without an entry.  Children are ordered by max
 *   leaf id as in src/node.cpp:32-59.
 *     unrooted tree: 2n-2 nodes (trifurcating root), parent_ids[2n-3],
 *                    branch_lengths[2n-2] (entry of the root unused).
 *     rooted tree:   2n-1 nodes, parent_ids[2n-2], branch_lengths[2n-1].
 *   Parameter rows follow BlockSpecification (src/block_specification.cpp:11-50,
 *   src/phylo_model.cpp:13-15): [GTR rates(6) | frequencies(4)] [Weibull shape]
 *   [clock rate]; query with mi_engine_block().
 *   All arrays are row-major, FP64 / int32, caller-owned.  Results come back in
 *   tree order.  Every function returns 0 on success; otherwise nonzero and
 *   mi_last_error() holds the message (the C++ adapter rethrows it as
 *   std::runtime_error, mirroring Failwith, src/sugar.hpp:67-78).
 *   An engine is not re-entrant (neither is the reference's, engine.hpp:26-54).
 *
 * Two families of entry points:
 *   mi_engine_*          host pointers in / host pointers out (what the cgo-like
 *                        binding in the reference would call)
 *   mi_engine_*_device   device pointers in / out, asynchronous on `stream`
 *                        (a hipStream_t passed as void*; NULL = the engine's own
 *                        stream).  Used by bench.py with inputs resident in HBM,
 *                        and by multi-GPU callers that hand results to RCCL.
 */
#ifndef MI_PHYLO_H_
#define MI_PHYLO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_PHYLO_ABI_VERSION 2

typedef struct mi_engine mi_engine;

enum { MI_SUBST_JC69 = 0, MI_SUBST_GTR = 1,         /* src/substitution_model.cpp:6-15 */
       MI_SUBST_REVERSIBLE = 2 };                     /* 20 states: empirical model given as data */
enum { MI_SITE_CONSTANT = 0, MI_SITE_WEIBULL = 1 }; /* src/site_model.cpp:10-25 */
enum { MI_CLOCK_NONE = 0, MI_CLOCK_STRICT = 1 };    /* src/clock_model.cpp:6-15 */

typedef struct {
  int32_t taxon_count;    /* n >= 3 */
  int32_t pattern_count;  /* P >= 1 */
  int32_t state_count;    /* s: 4 (DNA, everything the reference has) or 20 (amino acids) */
  int32_t category_count; /* K: 1 for constant, K of "weibull+K" */
  int32_t subst_model;    /* MI_SUBST_* */
  int32_t site_model;     /* MI_SITE_* */
  int32_t clock_model;    /* MI_CLOCK_* */
  int32_t use_tip_states; /* EngineSpecification::use_tip_states_, engine.hpp:20-24 */
  int32_t device;         /* HIP device ordinal; -1 = current device */
  int32_t reserved;
} mi_engine_spec;

int32_t mi_abi_version(void);
const char* mi_last_error(void);
/* visible HIP devices (0 without a GPU); what thread_count is capped by in the adapter */
int32_t mi_device_count(void);
/* bytes of device memory the library's own buffers hold in this process at the moment, engines'
 * and calls' (not the arrays mi_site_pattern_compress_device hands to the caller): back where it
 * was once every engine made since is destroyed, whatever other users of the device do */
int64_t mi_device_bytes_held(void);

/* Engine::Engine + FatBeagle::SetTipStates/SetTipPartials/SetPatternWeights.
 * tip_states[n*P]: 0..s-1, >= s means gap (src/site_pattern.cpp:16-46).
 * tip_partials[n*P*s] is read when use_tip_states == 0 (may be NULL: then the
 * partials are derived from tip_states exactly as SitePattern::GetPartials does,
 * src/site_pattern.cpp:117-131). */
int32_t mi_engine_create(const mi_engine_spec* spec, const int32_t* tip_states,
                         const double* tip_partials, const double* pattern_weights,
                         mi_engine** out_engine);
/* 20-state engines (state_count == 20, subst_model == MI_SUBST_REVERSIBLE; not in the
 * reference, whose factory src/substitution_model.cpp:6-15 knows JC69 and GTR only -- this is
 * the entry a third branch `"WAG"` of that factory would call).  The model is DATA with no
 * free parameters: 190 exchangeabilities (upper triangle, row by row, like the reference's
 * GTR rates, substitution_model.cpp:39-55) and 20 frequencies, amino-acid order
 * ARNDCQEGHILKMFPSTWYV; Q is built and normalised by the reference's GTR recipe and
 * eigendecomposed on the device once.  NULL tables = the built-in WAG table
 * (mi_engine_create does the same for such a spec).  tip_states: 0..19, >= 20 = gap /
 * ambiguous.  Parameter rows then hold only the site and clock blocks, as for JC69. */
int32_t mi_engine_create_reversible(const mi_engine_spec* spec, const double* exchangeabilities,
                                    const double* frequencies, const int32_t* tip_states,
                                    const double* tip_partials, const double* pattern_weights,
                                    mi_engine** out_engine);
/* One handle driving several devices -- what Engine's thread_count FatBeagles are
 * (src/engine.cpp:14-27; FatBeagleParallelize, src/fat_beagle.hpp:119-149): `shard_count`
 * engines, shard i on HIP device devices[i] (an ordinal may repeat, which puts several logical
 * shards on one device; a negative ordinal -1 - k means "the k-th device counting from the
 * caller's current HIP device, wrapping around"; NULL = {-1, -2, ...}: round-robin starting
 * at the current device, so that a one-process-per-GPU launch which selected its device with
 * hipSetDevice stays on it), tips and weights resident on each.  shard_mode MI_SHARD_TREES: the host-pointer calls deal the trees to
 * the shards in contiguous blocks (mi_shard_range), all devices work side by side, results
 * come back in tree order -- bit-identical to a single engine's.  MI_SHARD_PATTERNS (few
 * trees, very long alignments): shard i holds the site patterns mi_shard_range(P, count, i),
 * evaluates every tree on them, and the per-tree results of the unrooted calls (sums over
 * patterns, all of them) are added in shard order.  spec->device is ignored.
 * exchangeabilities / frequencies: as mi_engine_create_reversible (NULL for 4-state models).
 * The *_device entry points need a single-device engine (one engine per device, e.g. one
 * process per GPU under torch.distributed: INTEGRATION.md). */
enum { MI_SHARD_TREES = 0, MI_SHARD_PATTERNS = 1 };
int32_t mi_engine_create_sharded(const mi_engine_spec* spec, int32_t shard_count,
                                 const int32_t* devices, int32_t shard_mode,
                                 const double* exchangeabilities, const double* frequencies,
                                 const int32_t* tip_states, const double* tip_partials,
                                 const double* pattern_weights, mi_engine** out_engine);
int32_t mi_engine_shard_count(const mi_engine* engine);
/* The HIP device ordinal shard `shard` was placed on (a single-device engine: shard 0, its
 * device); -1 for an invalid argument.  What the -1 - k / NULL forms of `devices` resolved to:
 * the reference's counterpart is the thread a FatBeagle is pinned to, engine.cpp:23-27. */
int32_t mi_engine_shard_device(const mi_engine* engine, int32_t shard);
/* Contiguous block of shard `shard` of `shard_count` over `total` units: block sizes differ
 * by at most one, the larger blocks first. */
int32_t mi_shard_range(int32_t total, int32_t shard_count, int32_t shard, int32_t* begin,
                       int32_t* count);
/* the built-in WAG table in that form: exchangeabilities[190], frequencies[20] (sum 1) */
int32_t mi_wag_model(double* exchangeabilities, double* frequencies);
void mi_engine_destroy(mi_engine* engine);

/* Engine::GetPhyloModelBlockSpecification: blocks in std::map (ASCII) order. */
int32_t mi_engine_param_count(const mi_engine* engine);
int32_t mi_engine_block_count(const mi_engine* engine);
int32_t mi_engine_block(const mi_engine* engine, int32_t index, const char** name,
                        int32_t* start, int32_t* length);

/* ---- host-pointer entry points ------------------------------------------ */

/* Engine::LogLikelihoods(const UnrootedTreeCollection&, params, rescaling) */
int32_t mi_engine_log_likelihoods_unrooted(mi_engine* engine, int32_t tree_count,
                                           const int32_t* parent_ids,     /* [T][2n-3] */
                                           const double* branch_lengths,  /* [T][2n-2] */
                                           const double* params,          /* [T][param_count] */
                                           int32_t rescaling,
                                           double* out_log_likelihoods /* [T] */);

/* Engine::Gradients(const UnrootedTreeCollection&, ...): PhyloGradient per tree.
 * out_branch_gradient[T][2n-1] = gradient_["branch_lengths"] (last two entries 0);
 * out_site_gradient[T] = gradient_["site_model"] (K > 1, else untouched; may be NULL);
 * out_subst_gradient[T][8] = gradient_["substitution_model"] (GTR; may be NULL).
 * A NULL output also skips the work only it needs: without out_subst_gradient the 16
 * finite-difference log-likelihood passes of a GTR call (fat_beagle.cpp:400-465), without
 * out_site_gradient the separate site-model pass (fat_beagle.cpp:488-496); the outputs that
 * are delivered are bit-identical to those of the full call. */
int32_t mi_engine_gradients_unrooted(mi_engine* engine, int32_t tree_count,
                                     const int32_t* parent_ids, const double* branch_lengths,
                                     const double* params, int32_t rescaling,
                                     double* out_log_likelihoods, double* out_branch_gradient,
                                     double* out_site_gradient, double* out_subst_gradient);

/* Engine::Gradients(const UnrootedTreeCollection&, ...) followed, on the device, by the
 * reductions a variational-inference step applies to its result (vip/burrito.py:143-166,
 * vip/branch_model.py:104-133, src/unrooted_sbn_instance.cpp:176-198):
 *   out_sums[0] = sum_t w_t logL_t          out_sums[1] = sum_t w_t gradient_["site_model"]_t
 *   out_index_gradient[k] = sum over (t, v) with branch_index[t][v] == k of
 *                           w_t gradient_["branch_lengths"]_t[v]        (k < index_count)
 * branch_index[T][2n-1]: the parameter (split) index of every node's branch, negative = not a
 * parameter (the root and the fixed node always carry a zero gradient); tree_weights[T] or
 * NULL (w_t = 1).  Sums run in (t, v) order: deterministic.  out_log_likelihoods[T] may be
 * NULL.  A multi-GPU step then needs ONE all-reduce of 2 + index_count doubles.  The
 * substitution-model block (16 finite-difference passes for GTR) is not computed. */
int32_t mi_engine_gradients_unrooted_reduced(mi_engine* engine, int32_t tree_count,
                                             const int32_t* parent_ids,
                                             const double* branch_lengths, const double* params,
                                             int32_t rescaling, const int32_t* branch_index,
                                             const double* tree_weights, int32_t index_count,
                                             double* out_sums /* [2] */,
                                             double* out_index_gradient /* [index_count] */,
                                             double* out_log_likelihoods /* [T] or NULL */);

/* The diagonal of the branch-length Hessian of unrooted trees, per tree (an extension: no
 * counterpart in the reference's Engine).  For branch j of length t_j, with q the pre-order
 * vector at the bottom of the branch, L the post-order vector below it, Q the rate matrix and
 * category rates r_k, weights c_k: per pattern L_p = sum_k c_k q.L, D1_p = sum_k c_k r_k q.(Q L),
 * D2_p = sum_k c_k r_k^2 q.(Q^2 L), and
 *   out_branch_gradient[t][j]    = sum_p w_p D1_p / L_p                       (the gradient)
 *   out_branch_hessian[t][j]     = d^2 logL / d t_j^2 = sum_p w_p D2_p / L_p - S_j
 *   out_branch_gradient_sq[t][j] = S_j = sum_p w_p (D1_p / L_p)^2   (squared-derivative sum)
 * all [T][2n-1] in node-id order, the root and the fixed node (the last two entries) 0.  One
 * evaluation per tree with the tree's own model (a GTR engine: no finite-difference passes);
 * out_log_likelihoods, out_branch_gradient and out_branch_gradient_sq may be NULL.  The
 * log-likelihood and the gradient delivered are the gradient call's to 1e-12 relative.
 * 4-state engines only: a 20-state engine returns nonzero.  Sharded handles: MI_SHARD_TREES
 * deals the trees as the other calls do, results in tree order; MI_SHARD_PATTERNS adds all
 * four outputs (sums over patterns) in shard order. */
int32_t mi_engine_branch_hessian_unrooted(mi_engine* engine, int32_t tree_count,
                                          const int32_t* parent_ids,     /* [T][2n-3] */
                                          const double* branch_lengths,  /* [T][2n-2] */
                                          const double* params, int32_t rescaling,
                                          double* out_log_likelihoods /* [T] or NULL */,
                                          double* out_branch_gradient /* [T][2n-1] or NULL */,
                                          double* out_branch_hessian /* [T][2n-1] */,
                                          double* out_branch_gradient_sq /* [T][2n-1] or NULL */);

/* The NNI neighbourhood scan of unrooted trees (an extension: no counterpart in the reference's
 * Engine): the log-likelihood change of every nearest-neighbour interchange,
 * with the same model row and the same branch lengths, from one walk per tree.  In the
 * caller's tree (leaves 0..n-1, internal nodes in post-order, the trifurcating root 2n-3,
 * children ordered by largest leaf id) every internal node v with n <= v < 2n-3 is the lower
 * end of one inner edge.  Let (a, b) be v's children in child order, u its parent and c the
 * first, in child order, of u's children other than v (v's sibling; at the root the first of
 * the other two root children).
 *   neighbour 0 of v: v keeps a and takes c; b takes c's place under u
 *   neighbour 1 of v: v keeps b and takes c; a takes c's place under u
 * Every subtree carries the branch above it along, edge v keeps its length, nothing else
 * changes (mi_nni_neighbour builds these trees).
 *   out_nni_delta[t][v][i] = logL(neighbour i of v) - logL(tree t) = sum_p w_p log(L'_p / L_p)
 * per pattern, not a difference of two totals; [T][2n-1][2] by node id, 0 for leaves, 2n-3 and
 * 2n-2.  out_best_move[t] = 2 v + i of the largest delta, the lowest code among equals, -1 when
 * n == 3.  out_log_likelihoods is that of a gradient call on the HBM path, bit for bit.  One
 * evaluation per tree with the tree's own model (a GTR engine: no finite-difference passes).
 * 4-state engines only: a 20-state engine returns nonzero.  Sharded handles: MI_SHARD_TREES
 * deals the trees as the other calls do, results in tree order; MI_SHARD_PATTERNS adds logL
 * and delta (sums over patterns) in shard order and takes the best move from the sums. */
int32_t mi_engine_nni_scan_unrooted(mi_engine* engine, int32_t tree_count,
                                    const int32_t* parent_ids,     /* [T][2n-3] */
                                    const double* branch_lengths,  /* [T][2n-2] */
                                    const double* params, int32_t rescaling,
                                    double* out_log_likelihoods /* [T] or NULL */,
                                    double* out_nni_delta /* [T][2n-1][2] */,
                                    int32_t* out_best_move /* [T] or NULL */);
/* Neighbour `which` (0 | 1) of inner edge `node` of ONE tree, as defined above, renumbered in
 * the reference's convention, every branch length moved to its subtree's new id (the entry of
 * the root, 2n-3, is copied).  Pure host arithmetic: no device is touched.  Nonzero when
 * `node` is not the lower end of an inner edge, `which` is neither 0 nor 1, or the parent-id
 * vector is not a tree in the reference's form. */
int32_t mi_nni_neighbour(int32_t taxon_count, const int32_t* parent_ids /* [2n-3] */,
                         const double* branch_lengths /* [2n-2] */, int32_t node, int32_t which,
                         int32_t* out_parent_ids /* [2n-3] */, double* out_branch_lengths /* [2n-2] */);

/* Per-pattern log-likelihoods of unrooted trees (an extension: what RELL bootstrap, expected-
 * likelihood weights and the KH / SH / AU tests start from).
 *   out_pattern_log_likelihoods[t][p] = log L_p(tree t), UNWEIGHTED: the pattern weight is not
 * applied and patterns of weight 0 are reported like the others.  With rescaling it is
 * log(mantissa) + exponent ln 2, the expression the log-likelihood kernels sum.  A pattern of
 * likelihood 0 gives -inf (IEEE; not trapped).  A pattern in which every tip vector is all ones
 * (an all-gap column) has likelihood 1 whatever the tree and is reported as exactly 0.0 (the
 * log-likelihood call's arithmetic leaves it a few units of 2^-53 off, which the sums keep).  out_log_likelihoods is what
 * mi_engine_log_likelihoods_unrooted returns for the same inputs, bit for bit: the call takes
 * the log-likelihood call's route (MI_PHYLO_LOGLIK_PATH included) with the PATTERN_LL variant
 * of its kernel, one evaluation per tree with the tree's own model row (a GTR engine: no
 * finite-difference passes).  mi_engine_last_call_path is the log-likelihood call's line with
 * the token " pattern_ll".  4-state engines only: a 20-state engine returns nonzero.  Sharded
 * handles: MI_SHARD_TREES deals the trees as the other calls do, rows in tree order;
 * MI_SHARD_PATTERNS is refused (each shard holds a block of columns). */
int32_t mi_engine_pattern_log_likelihoods_unrooted(mi_engine* engine, int32_t tree_count,
                                                   const int32_t* parent_ids,     /* [T][2n-3] */
                                                   const double* branch_lengths,  /* [T][2n-2] */
                                                   const double* params, int32_t rescaling,
                                                   double* out_log_likelihoods /* [T] or NULL */,
                                                   double* out_pattern_log_likelihoods /* [T][P] */);

/* Marginal ancestral-state and rate-category posteriors per pattern (an extension: no
 * counterpart in the reference's Engine), from one post-order and pre-order
 * walk per tree.  The tree is unrooted, in the caller's form: leaves 0..n-1, internal nodes
 * n..2n-3 in post-order, the trifurcating root 2n-3.  The model has 4 states, K categories with
 * weights c_k and rates r_k and stationary frequencies pi.  For an internal node v below the
 * root L_v,k is the post-order vector at v and q_v,k the pre-order vector at the bottom of the
 * branch above v (the Hessian call's convention: L_p = sum_k c_k q . L at every branch); at the
 * root q = pi and L is the product of the three child messages.  Per tree t and pattern p:
 *   J[v][s]                          = sum_k c_k q_v,k[s] L_v,k[s]
 *   out_state_posteriors[t][v-n][p][s] = J[v][s] / sum_s' J[v][s']        v = n .. 2n-3
 *   out_map_state[t][v-n][p]         = the s of the largest posterior, the lowest among equals
 *   C[k]                             = c_k sum_s pi_s L_root,k[s]
 *   out_category_posteriors[t][p][k] = C[k] / sum_k' C[k']
 *   out_pattern_rate[t][p]           = sum_k r_k out_category_posteriors[t][p][k]
 *   out_tip_posteriors[t][v][p][s]   = (q_v o L_v) normalised in the same way at the leaves
 *                                      v = 0 .. n-1: the tip vector itself for an unambiguous
 *                                      tip, an imputation for gaps, 0/1 masks and tip partials
 * The denominator is the sum of the numerators as computed (the pattern likelihood from
 * elsewhere is not used), so a row sums to 1 to rounding.  Under rescaling one power of two is
 * removed per node and pattern across all categories; it sits in every numerator alike and
 * cancels: rescaled and unrescaled results agree to rounding, not bit for bit.  Values are
 * unweighted; patterns of weight 0 are reported like the others.  A pattern of likelihood 0
 * gives NaN rows (0/0) and map state 0.  K = 1 gives category posterior 1 exactly and
 * out_pattern_rate = r_0.  out_log_likelihoods is that of a gradient call on the HBM path, bit
 * for bit.  One evaluation per tree with the tree's own model row (a GTR engine: no
 * finite-difference passes).  Only out_state_posteriors is required; every other output may be
 * NULL and then costs no work.  4-state engines only: a 20-state engine returns nonzero.
 * Sharded handles: MI_SHARD_TREES deals the trees as the other calls do, rows in tree order;
 * MI_SHARD_PATTERNS is refused (each shard holds a block of columns). */
int32_t mi_engine_ancestral_states_unrooted(mi_engine* engine, int32_t tree_count,
                                            const int32_t* parent_ids,     /* [T][2n-3] */
                                            const double* branch_lengths,  /* [T][2n-2] */
                                            const double* params, int32_t rescaling,
                                            double* out_log_likelihoods /* [T] or NULL */,
                                            double* out_state_posteriors /* [T][n-2][P][4] */,
                                            int8_t* out_map_state /* [T][n-2][P] or NULL */,
                                            double* out_category_posteriors /* [T][P][K] or NULL */,
                                            double* out_pattern_rate /* [T][P] or NULL */,
                                            double* out_tip_posteriors /* [T][n][P][4] or NULL */);

/* Phylogenetic placement (an extension: no counterpart in the reference's Engine; DESIGN.md
 * 4.17): score Q query sequences on every edge of trees that are already built.  The trees are
 * unrooted, in the caller's form; edge e = 0 .. 2n-4 is the branch above node e, of length
 * t_e = branch_lengths[e] (the root 2n-3 has none): E = 2n-3 edges.  Placing a query on e with
 * pendant length l is the tree on n+1 taxa in which a new node splits e into two halves of
 * length t_e / 2 and the query hangs from that node by a branch of length l, under the tree's own
 * model row and rate categories.  Only the midpoint is scored.  With g_e,k the pre-order vector
 * at the top of e (it carries pi), L_e,k the post-order vector at its bottom, H = P(r_k t_e / 2)
 * and R_g,k = P(r_k l_g), per tree t, edge e, pendant length g and pattern p:
 *   M_e,k[j]         = (H^T g_e,k)[j] (H L_e,k)[j]
 *   Z[a]             = sum_k c_k sum_j M_e,k[j] R_g,k[j][a]                 a = 0..3
 *   S[t][e][g][a][p] = s[t][p] + log(Z[a] / ((Z[0] + Z[1]) + (Z[2] + Z[3])))  a = 0..3
 *   S[t][e][g][4][p] = s[t][p]                                              a gap: any code >= 4
 * s[t][p] is the per-pattern log-likelihood of the tree as the call's post-order pass forms it.
 * Powers of two that rescaling removed sit in numerator and denominator alike and cancel.
 * A query is a row of compact states x[q][c] over C columns (0..3; anything else is a gap);
 * column_pattern[c] in [0, P) names the engine pattern column c extends; column_weights[c]
 * (NULL: 1) weighs it.
 *   ll[t][q][e][g]   = sum_c column_weights[c] S[t][e][g][x[q][c]][column_pattern[c]]
 *   edge_ll[t][q][e] = max_g ll,  pendant_index[t][q][e] = the lowest such g
 *   best_edge[t][q]  = the e of the largest edge_ll, the lowest among equals
 *   lwr[t][q][e]     = exp(edge_ll - m) / sum_e' exp(edge_ll[e'] - m),  m = max_e edge_ll
 *                      (likelihood weight ratio; the sum in ascending e')
 * Columns of weight 0 are skipped whatever their table entry.  A table entry of -inf (pendant
 * length 0 on a zero-length leaf edge of another state) propagates as IEEE says.
 * THE ORDER of every sum ll[t][q][e][g] is fixed and depends on C alone -- not on Q, E, G, T, the
 * place of the (query, edge) pair in a launch, how the call was cut into launches, or where the
 * table was read from: 64 running sums, number l taking the columns c = l, l + 64, l + 128, ...
 * in ascending c, each term by one fused multiply-add fma(w_c, S, sum) from +0.0; then the 64
 * are added pairwise by an xor butterfly: v[i] += v[i ^ 32], then ^ 16, 8, 4, 2, 1 (every
 * position ends with the same value).  Equal query rows give bit-identical output rows; there
 * are no floating-point atomics.
 * 1 <= pendant_count <= MI_PLACEMENT_MAX_PENDANTS, every pendant length finite and >= 0;
 * query_count >= 1, column_count >= 1.  out_log_likelihoods is that of a gradient call on the HBM
 * path, bit for bit.  Only out_edge_log_likelihoods is required; a NULL output costs neither
 * arithmetic nor stores.  4-state engines and unrooted trees only.  Sharded handles:
 * MI_SHARD_TREES deals the trees, rows in tree order, every shard gets all queries;
 * MI_SHARD_PATTERNS is refused (each shard holds a block of columns).  The table workspace
 * counts against MI_PHYLO_PLV_BYTES: a batch over the budget is cut into launches over trees and
 * writes the same bytes; one tree's table over the budget is refused. */
#define MI_PLACEMENT_MAX_PENDANTS 4
int32_t mi_engine_placement_unrooted(mi_engine* engine, int32_t tree_count,
                                     const int32_t* parent_ids,     /* [T][2n-3] */
                                     const double* branch_lengths,  /* [T][2n-2] */
                                     const double* params, int32_t rescaling, int32_t query_count,
                                     int32_t column_count, const int8_t* query_states /* [Q][C] */,
                                     const int32_t* column_pattern /* [C] */,
                                     const double* column_weights /* [C] or NULL */, int32_t pendant_count,
                                     const double* pendant_lengths /* [G] */,
                                     double* out_log_likelihoods /* [T] or NULL */,
                                     double* out_edge_log_likelihoods /* [T][Q][2n-3] */,
                                     int8_t* out_pendant_index /* [T][Q][2n-3] or NULL */,
                                     int32_t* out_best_edge /* [T][Q] or NULL */,
                                     double* out_lwr /* [T][Q][2n-3] or NULL */,
                                     double* out_edge_tables /* [T][2n-3][G][5][P] or NULL */);

/* The SPR neighbourhood scan (an extension: no counterpart in the reference's Engine; DESIGN.md
 * 4.18): for trees at given branch lengths, the log-likelihood change of every subtree-prune-and-
 * regraft move "cut this edge, re-attach the loose part on the midpoint of that edge".  The trees
 * are unrooted, in the caller's form: leaves 0..n-1, internal nodes in post-order, trifurcating
 * root 2n-3; edge e = 0 .. 2n-4 is the branch above node e, of length t_e; E = 2n-3 edges.
 * A move is (s, dir, f).
 * dir = 0, the clade moves: edge s is cut at its top; clade s keeps its branch of length t_s.
 *   The parent u of s is removed.  If u is not the root, its other child y and the edge above u
 *   become one edge of length t_y + t_u; if u is the root, with other children y1 and y2, these
 *   are joined by one edge of length t_y1 + t_y2.  The target edge f of the remaining tree is
 *   split at its midpoint, both halves t_f / 2, and the clade is hung there on its branch t_s.
 *   Valid targets: every edge that is none of s, an edge inside clade s, y and u (at the root:
 *   y1, y2) -- those two name the merged edge and would give the topology back.
 * dir = 1, the rest moves: s must be an internal node, with children a and b.  Edge s is cut at
 *   its bottom; everything outside clade s keeps the branch t_s.  Node s is removed, a and b are
 *   joined by an edge of length t_a + t_b.  The target f is an edge strictly inside clade a or
 *   clade b, split at its midpoint, and the rest is hung there on t_s.  A leaf s has no dir = 1
 *   moves.
 * Distance and radius: the distance of a move is the number of nodes of the pruned tree on the
 * path between the merged edge and f; the edges touching the merged edge are at distance 1.
 * radius >= 1 keeps the moves of distance <= radius, radius = 0 keeps all; a negative radius is
 * refused.
 * The gain: delta[t][s][dir][f] = logL(neighbour) - logL(tree t), under the same model row and
 * the branch lengths just described, formed per pattern as sum_p w_p log(L'_p / L_p), never as a
 * difference of two totals (patterns of weight 0 are skipped).
 * Outputs:
 *   out_log_likelihoods [T] (or NULL): bit for bit the gradient call's on the HBM path
 *   out_best_target [T][E][2] (int32), out_best_delta [T][E][2]: per (s, dir) the target of the
 *     largest delta, the lowest f among equals; -1 and -inf where (s, dir) has no valid move
 *     within the radius
 *   out_best_move [T][3] (or NULL): (s, dir, f) of the largest delta of the tree, among equals
 *     the lowest code (2 s + dir) E + f; (-1, -1, -1) where the tree has no move (n = 3)
 *   out_delta [T][E][2][E] (or NULL): the whole table; every entry that is no valid move within
 *     the radius is -inf
 * Sums over patterns are formed tile by tile in one fixed order: a tree's outputs do not depend
 * on the batch it came in or on how the call was cut into launches.  4-state engines and
 * unrooted trees only.  Sharded handles: MI_SHARD_TREES deals the trees; MI_SHARD_PATTERNS is
 * refused.  The scan's workspace (a second vector arena, rescaling exponents, the per-tile table)
 * counts against MI_PHYLO_PLV_BYTES: a batch over the budget is cut into launches over trees and
 * writes the same bytes; one tree's workspace over the budget is refused. */
int32_t mi_engine_spr_scan_unrooted(mi_engine* engine, int32_t tree_count,
                                    const int32_t* parent_ids,    /* [T][2n-3] */
                                    const double* branch_lengths, /* [T][2n-2] */
                                    const double* params, int32_t rescaling, int32_t radius,
                                    double* out_log_likelihoods /* [T] or NULL */,
                                    int32_t* out_best_target /* [T][2n-3][2] */,
                                    double* out_best_delta /* [T][2n-3][2] */,
                                    int32_t* out_best_move /* [T][3] or NULL */,
                                    double* out_delta /* [T][2n-3][2][2n-3] or NULL */);

/* The tree the move (s, dir, f) of mi_engine_spr_scan_unrooted leads to, in the reference's
 * numbering: leaves keep their ids, internal nodes in post-order, children ordered by largest
 * leaf id.  It is rooted at the caller's root node if that node survives, else (dir = 0 with
 * parent(s) the root) at the new attachment node.  Every length goes with its edge (edges on a
 * reversed path carry their length along); the merged edge is t_y + t_u, the halves 0.5 * t_f;
 * the entry of 2n-3 is copied.  Host arithmetic only.  Nonzero for a triple that is no valid move
 * (any radius) or a parent-id vector that is no tree. */
int32_t mi_spr_neighbour(int32_t taxon_count, const int32_t* parent_ids /* [2n-3] */,
                         const double* branch_lengths /* [2n-2] */, int32_t s, int32_t dir, int32_t f,
                         int32_t* out_parent_ids /* [2n-3] */, double* out_branch_lengths /* [2n-2] */);

/* RELL re-summation (resampling of estimated log-likelihoods) and its reductions (an extension;
 * DESIGN.md 4.12), for B replicates, T trees and P patterns -- P is an argument: any engine
 * serves (the alignment plays no part), a sharded handle lets its first shard do it.
 *   C[b][t]  = sum_p W[b][p] s[t][p]       (FP64 matrix cores)
 *   best[b]  = the tree of the largest C[b][.], the lowest index among equals
 *   bp[t]    = (double)#{b : best[b] = t} / B
 *   elw[t]   = (1/B) sum_b exp(C[b][t] - m_b) / sum_t' exp(C[b][t'] - m_b),  m_b = max_t C[b][t]
 * Determinism is part of the interface: every C[b][t] is accumulated over p in one fixed order
 * (ascending, four patterns per step, one accumulator) that depends neither on B, T nor on
 * where the pair falls in the launch -- equal rows of s give bit-identical columns of C --; the
 * reductions use fixed trees and ordered sums; no floating-point atomics anywhere. */
int32_t mi_engine_rell(mi_engine* engine, int32_t replicate_count, int32_t tree_count,
                       int32_t pattern_count, const double* pattern_log_likelihoods /* [T][P] */,
                       const double* replicate_weights /* [B][P] */,
                       double* out_replicate_log_likelihoods /* [B][T] or NULL */,
                       int32_t* out_best_tree /* [B] or NULL */,
                       double* out_bootstrap_proportion /* [T] */,
                       double* out_expected_likelihood_weight /* [T] or NULL */);

/* The common case in one host call: upload, mi_engine_pattern_log_likelihoods_unrooted,
 * mi_engine_rell with the engine's pattern count, download -- nothing returns to the host in
 * between.  Sharded handles of more than one shard are refused (the product needs every
 * tree's row on one device). */
int32_t mi_engine_rell_bootstrap_unrooted(mi_engine* engine, int32_t tree_count,
                                          const int32_t* parent_ids,     /* [T][2n-3] */
                                          const double* branch_lengths,  /* [T][2n-2] */
                                          const double* params, int32_t rescaling,
                                          int32_t replicate_count,
                                          const double* replicate_weights /* [B][P] */,
                                          double* out_log_likelihoods /* [T] */,
                                          double* out_pattern_log_likelihoods /* [T][P] or NULL */,
                                          double* out_replicate_log_likelihoods /* [B][T] or NULL */,
                                          int32_t* out_best_tree /* [B] or NULL */,
                                          double* out_bootstrap_proportion /* [T] */,
                                          double* out_expected_likelihood_weight /* [T] or NULL */);

/* The marginal of a mixture of trees from their per-pattern log-likelihoods (an extension;
 * DESIGN.md 4.12):
 *   out_pattern_log_marginal[p] = logsumexp_t(s[t][p] + tree_log_weights[t])
 *   out_log_marginal[0]         = sum_p pattern_weights[p] out_pattern_log_marginal[p]
 * tree_log_weights NULL: log(1/T) each.  t in ascending order after a maximum pass, the final
 * sum in a fixed order.  Any engine serves, as for mi_engine_rell. */
int32_t mi_engine_pattern_mixture(mi_engine* engine, int32_t tree_count, int32_t pattern_count,
                                  const double* pattern_log_likelihoods /* [T][P] */,
                                  const double* tree_log_weights /* [T] or NULL */,
                                  const double* pattern_weights /* [P] */,
                                  double* out_pattern_log_marginal /* [P] */,
                                  double* out_log_marginal /* [1] */);

/* Replicate weights of a (multiscale) bootstrap, drawn on the device (an extension).
 * Any engine serves: P is an argument.  pattern_weights [P] must be non-negative integer site
 * counts with N = sum in [1, 2^31); `sites` = n in [1, 2^33] is the number of draws per replicate
 * (n = N: the ordinary bootstrap; another n: a scaled replicate of the AU test).  The output
 * W [B][P] (float64) is what mi_engine_rell, mi_engine_pairwise_distances and
 * mi_engine_starting_trees_unrooted take as replicate_weights.
 *
 * The definition is part of the interface and integer-exact: a row's bits depend on (seed,
 * replicate number, n, pattern_weights) alone.  For replicate number rho = first_replicate + b,
 * Philox4x32-10 call j = 0 .. ceil(n/2) - 1 has key (seed lo, seed hi) and counter
 * (j, 0x72656C6C, rho lo, rho hi) -- the fixed second word keeps the stream apart from
 * mi_engine_sbn_sample's and mi_engine_branch_model_sample's -- and yields c0..c3: draw 2j is
 * x = c0 2^32 + c1, draw 2j+1 is x = c2 2^32 + c3 (unused when n is odd).  The site of a draw is
 * (x N) >> 64 (the high word of the 64 x 64 product), its pattern the p with cum[p] <= site <
 * cum[p+1], cum the exclusive integer prefix sum of the weights; W[b][p] counts the draws that
 * landed in p (a zero-weight pattern is never drawn).  A count of 2^32 or more wraps. */
int32_t mi_engine_bootstrap_weights(mi_engine* engine, int32_t pattern_count,
                                    const double* pattern_weights /* [P] */, int32_t replicate_count,
                                    int64_t sites, uint64_t seed, int64_t first_replicate,
                                    double* out_replicate_weights /* [B][P] */);

/* The KH, SH and AU tests with BP and ELW for T trees from their per-pattern log-likelihoods
 * s [T][P] and the pattern weights w [P] (an extension; any engine serves).
 * K blocks (1 <= K <= MI_TOPOLOGY_MAX_SCALES) of replicates[k] >= 1 replicates with sites[k] draws
 * each: sites[0] must equal N = sum w, the sites pairwise distinct.  Block k draws its weights as
 * mi_engine_bootstrap_weights does, replicate numbers continuing from block to block
 * (first_replicate + sum_{j<k} replicates[j]), forms C_k = W_k s^T and counts the replicates each
 * tree wins, counts[k][t], exactly as mi_engine_rell does; one workspace sized by the largest
 * block serves them in turn.  L = s w through the same product.  From block 0 (B, C):
 *   bp, elw    as mi_engine_rell gives them
 *   t1, t2     argmax_t L and the argmax over the others, the lowest index among equals
 *   mean[t]    (sum_b C[b][t]) / B, one accumulator, b ascending;  Z[b][t] = C[b][t] - mean[t]
 *   p_SH[t]    #{b : max_t' Z[b][t'] - Z[b][t] >= L[t1] - L[t]} / B
 *   p_KH[t]    #{b : Z[b][ref] - Z[b][t] >= L[ref] - L[t]} / B, ref = t1 (t != t1), t2 (t = t1);
 *              one tree: 1
 * AU per tree over the usable blocks (0 < counts[k][t] < replicates[k]), in block order: with
 * r = sites[k] / N, pi = counts[k][t] / replicates[k], z = -Phi^-1(pi), omega = replicates[k]
 * phi(z)^2 / (pi (1 - pi)), the weighted least-squares fit z ~ d sqrt(r) + c / sqrt(r);
 * p_AU = Phi(c - d), rss = sum omega (z - d sqrt(r) - c / sqrt(r))^2; fewer than two usable
 * blocks: p_AU = bp, d = c = rss = NaN.
 * out_table [T][MI_TOPOLOGY_COLUMNS], per tree: L | L[t1] - L | bp | elw | p_KH | p_SH | p_AU | d |
 * c | rss | usable blocks.  Counts are integers (integer atomics, ordered sums); no float atomics. */
#define MI_TOPOLOGY_MAX_SCALES 64
#define MI_TOPOLOGY_COLUMNS 11
int32_t mi_engine_topology_tests(mi_engine* engine, int32_t tree_count, int32_t pattern_count,
                                 const double* pattern_log_likelihoods /* [T][P] */,
                                 const double* pattern_weights /* [P] */, int32_t block_count,
                                 const int64_t* sites /* [K], host */, const int32_t* replicates /* [K], host */,
                                 uint64_t seed, int64_t first_replicate,
                                 double* out_table /* [T][MI_TOPOLOGY_COLUMNS] */,
                                 int32_t* out_counts /* [K][T] */, double* out_mean /* [T] or NULL */,
                                 double* out_replicate_log_likelihoods /* [B_0][T] or NULL */,
                                 int32_t* out_best_tree /* [B_0] or NULL */);

/* From trees to the table in one host call: upload, mi_engine_pattern_log_likelihoods_unrooted,
 * mi_engine_topology_tests with the engine's own pattern weights, one download.  Support as
 * mi_engine_rell_bootstrap_unrooted: 4-state engines; a handle of more than one shard and a
 * pattern-sharded handle are refused; engine weights that are no integer site counts are refused. */
int32_t mi_engine_topology_tests_unrooted(mi_engine* engine, int32_t tree_count,
                                          const int32_t* parent_ids,     /* [T][2n-3] */
                                          const double* branch_lengths,  /* [T][2n-2] */
                                          const double* params, int32_t rescaling, int32_t block_count,
                                          const int64_t* sites /* [K] */, const int32_t* replicates /* [K] */,
                                          uint64_t seed, int64_t first_replicate,
                                          double* out_log_likelihoods /* [T] */,
                                          double* out_pattern_log_likelihoods /* [T][P] or NULL */,
                                          double* out_table /* [T][MI_TOPOLOGY_COLUMNS] */,
                                          int32_t* out_counts /* [K][T] */, double* out_mean /* [T] or NULL */,
                                          double* out_replicate_log_likelihoods /* [B_0][T] or NULL */,
                                          int32_t* out_best_tree /* [B_0] or NULL */);

/* Starting trees from the engine's alignment (an extension; 4-state engines):
 * pairwise maximum-likelihood distances for B sets of pattern weights, neighbour joining of B
 * distance matrices, and the two in one call.  With the replicate weights of a bootstrap
 * (what RELL resamples with) B distance matrices give B neighbour-joining trees: a batch of
 * starts for mi_engine_nni_search_unrooted, and a distance bootstrap.
 *
 * Counts.  For taxa i < j and states a, b
 *   N_r[i][j][a][b] = sum_p W[r][p] [tip_i(p) = a] [tip_j(p) = b]     (FP64 matrix cores)
 * A tip counts as state a when its compact code is a or -- an engine made from tip partials --
 * its vector is exactly the unit vector e_a; every other tip (gap, 0/1 mask, real-valued
 * partial) is missing, and a pattern with a missing tip at i or j adds nothing to that pair
 * (pairwise deletion).  Every count has one accumulator that takes the patterns in ascending
 * order, four per step, from p = 0, whatever B, n and the pair's place in the launch: with
 * integer weights the counts are exact, and equal rows of W give bit-identical counts and
 * distances.  replicate_weights NULL: one replicate, the engine's pattern weights.  The weights
 * must be finite (they are not checked: a non-finite one makes NaN counts).
 *
 * Distance.  With the rates r_k and weights c_k of the model row's site model and P(.) of its
 * substitution model (ONE row params[param_count] for the call),
 *   d = argmax over t in [min_length, max_length] of l(t) = sum_ab N[a][b] log sum_k c_k P_ab(r_k t)
 * by a safeguarded Newton iteration on l': a bracket kept by the sign of l', a step that
 * leaves it (one that lands on an end has not) or an l'' >= 0 replaced by the bracket's
 * midpoint, started at the JC69 closed form
 * of the pair's mismatch share clamped into the box, stopped when |step| <= tolerance max(t, 1e-3)
 * or after max_iterations.  l'(min_length) <= 0 gives min_length, l'(max_length) >= 0
 * max_length, a pair with no comparable pattern (sum N = 0) max_length.
 *   out_distances   [B][n][n]            symmetric, zero diagonal
 *   out_pair_counts [B][n(n-1)/2][16]    or NULL; pairs in lexicographic (i, j) order, 4 a + b
 *   out_pair_status [B][n(n-1)/2]        or NULL; MI_DISTANCE_*
 * The counts of B replicates are worked off in chunks that keep the count workspace within
 * MI_PHYLO_PLV_BYTES (mi_engine_last_call_launches: the chunks; mi_engine_last_call_path:
 * "pair_counts B=<B> chunks=<c>").  Sharded handles: a tree-sharded handle lets its first shard
 * do the work (every shard holds the whole alignment); MI_SHARD_PATTERNS is refused. */
enum {
  MI_DISTANCE_CONVERGED = 0,
  MI_DISTANCE_LOWER_BOUND = 1,
  MI_DISTANCE_UPPER_BOUND = 2,
  MI_DISTANCE_NO_DATA = 3,
  MI_DISTANCE_ITERATION_LIMIT = 4
};
typedef struct {
  int32_t max_iterations; /* Newton iterations per pair, 1..1000 (default 50) */
  int32_t reserved0;      /* 0 */
  double tolerance;       /* default 1e-10 */
  double min_length;      /* default 1e-8 */
  double max_length;      /* default 10 */
  int32_t reserved[4];    /* 0 */
} mi_distance_options;    /* a field left at 0 takes its default */
int32_t mi_engine_pairwise_distances(mi_engine* engine, int32_t replicate_count,
                                     const double* replicate_weights /* [B][P] or NULL */,
                                     const double* params /* [param_count] */,
                                     const mi_distance_options* options /* NULL: the defaults */,
                                     double* out_distances /* [B][n][n] */,
                                     double* out_pair_counts /* [B][n(n-1)/2][16] or NULL */,
                                     int8_t* out_pair_status /* [B][n(n-1)/2] or NULL */);

/* Neighbour joining (Saitou & Nei) of B distance matrices [B][n][n], of which only i < j is
 * read; n is an argument: any engine serves (the alignment plays no part), a sharded handle
 * lets its first shard do it.  The trees come in the form every unrooted call takes: leaves
 * 0..n-1, internal nodes in post-order with the children ordered by largest leaf id, the
 * trifurcating root 2n-3, its length entry 0.  The rule, so that it is reproducible: clusters
 * live in slots 0..n-1; joining slots i < j puts the new cluster in slot i and kills slot j;
 * with r live slots and R_i = sum_k d(i, k) over the live slots in ascending order, the pair
 * that minimises Q(i, j) = (r-2) d(i, j) - R_i - R_j is joined, the lowest (i, j) among equals;
 * delta_i = d(i, j) / 2 + (R_i - R_j) / (2 (r-2)), delta_j = d(i, j) - delta_i,
 * d(u, k) = (d(i, k) + d(j, k) - d(i, j)) / 2; the last three clusters a < b < c hang under the
 * root with (d_ab + d_ac - d_bc) / 2 and its two rotations; n = 3 is that step alone.  Every
 * operation is rounded once, in the order written (the kernel is compiled without
 * floating-point contraction), so a host implementation in IEEE doubles gives the same bits.  The lengths are clamped into
 * [min_length, max_length] on their way out (raw lengths can be negative), never in the
 * matrix.  A distance that is not finite is an error that names its matrix ("... (matrix b)").
 * mi_engine_last_call_path: "nj n=<n> store=lds|global". */
int32_t mi_engine_neighbour_joining(mi_engine* engine, int32_t replicate_count, int32_t taxon_count,
                                    const double* distances /* [B][n][n] */, double min_length,
                                    double max_length, int32_t* out_parent_ids /* [B][2n-3] */,
                                    double* out_branch_lengths /* [B][2n-2] */);

/* mi_engine_pairwise_distances followed by mi_engine_neighbour_joining (clamped into the
 * options' box) on the engine's alignment; nothing returns to the host in between.
 * out_distances may be NULL.  The results are those of the two calls, bit for bit. */
int32_t mi_engine_starting_trees_unrooted(mi_engine* engine, int32_t replicate_count,
                                          const double* replicate_weights /* [B][P] or NULL */,
                                          const double* params /* [param_count] */,
                                          const mi_distance_options* options /* NULL: the defaults */,
                                          int32_t* out_parent_ids /* [B][2n-3] */,
                                          double* out_branch_lengths /* [B][2n-2] */,
                                          double* out_distances /* [B][n][n] or NULL */);

/* ---- split tables of tree batches (an extension) ----
 *
 * Trees: n taxa, leaves 0..n-1, internal nodes in post-order, the root 2n-3 of degree 3 -- the
 * form every unrooted call takes.  Edge v is the branch above node v, v < 2n-3.  The SPLIT of
 * edge v is the set of leaves below v, minorised as the reference does (Bitset::Minorize,
 * src/bitset.cpp:147-152): if it holds taxon 0, its complement is taken, so a split never holds
 * taxon 0.  A split is stored as W = ceil(n/32) uint32 words, taxon i in bit i & 31 of word
 * i >> 5; bits at and above n are 0, also after a complement.  The distinct splits of a batch
 * are numbered BY FIRST OCCURRENCE in (t, v) order: the index of a split is the number of
 * distinct splits whose first occurrence comes earlier.  So the trivial split of leaf v has
 * index v (tree 0's leaves come first) and the nontrivial splits start at n; the indices of
 * trees 0..t do not change when trees are appended; a tree put first has index v on its edge v.
 * (The reference's own numbering is its unordered_map's iteration order and depends on the
 * compiler, unrooted_sbn_instance.hpp:120-121: it is not reproduced.)  A split occurs at most
 * once per tree.  A parent-id vector that is not a tree in that form, a root of degree 2
 * included, is an error that names its tree ("... (tree t)").
 *
 * mi_engine_split_index: the table.  taxon_count is an argument: any engine serves, 4 or 20
 * states (the alignment plays no part); a sharded handle lets its first shard do the work.
 *   out_split_index [T][2n-1]      index of the split of edge v; -1 in entries 2n-3 and 2n-2:
 *                                  the layout and the "negative = not a parameter" rule of
 *                                  mi_engine_gradients_unrooted_reduced's branch_index
 *   out_split_count [1]            S, the number of distinct splits
 *   out_split_bits  [capacity][W]  the split
 *   out_split_first [capacity]     entry number t (2n-1) + v of its first occurrence
 *   out_split_trees [capacity]     number of trees that hold it
 *   out_split_stats [capacity][3] or NULL: sum w_t, sum round(w_t l), sum round(w_t round(l l))
 *                                  over the trees that hold it IN ASCENDING TREE ORDER, one
 *                                  accumulator each, every operation rounded once (l: that
 *                                  tree's length of the edge; columns 1 and 2 are 0 without
 *                                  branch_lengths; w = 1 without tree_weights).  Support, mean
 *                                  and variance of a split's length follow (what the reference's
 *                                  PSPIndexer::SplitLengths is used for, src/psp_indexer.cpp:110-120)
 * Rows at and above S are left untouched.  S > split_capacity is an error whose message carries
 * S; T (2n-3) always suffices.  The workspace is (4 W + 16) bytes per occurrence (an edge of a
 * tree) plus 12 bytes per slot of a table of the power of two at or above twice the occurrences,
 * 16 more bytes per occurrence and a sort's temporary storage when statistics are asked for,
 * and 512 (n-1) bytes per wave of trees beyond 128 taxa.  The call is NOT chunked: a batch whose
 * workspace is over MI_PHYLO_PLV_BYTES is refused with the sizes in the message.
 * mi_engine_last_call_path: "splits n=<n> W=<W> store=lds|global". */
int32_t mi_engine_split_index(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                              const int32_t* parent_ids /* [T][2n-3] */,
                              const double* branch_lengths /* [T][2n-2] or NULL */,
                              const double* tree_weights /* [T] or NULL */, int32_t split_capacity,
                              int32_t* out_split_index /* [T][2n-1] */, int32_t* out_split_count /* [1] */,
                              uint32_t* out_split_bits /* [capacity][W] */,
                              int32_t* out_split_first /* [capacity] */,
                              int32_t* out_split_trees /* [capacity] */,
                              double* out_split_stats /* [capacity][3] or NULL */);

/* Distances between the trees of a batch from their split indices (any array in the layout
 * above: entries 0..2n-4 of a row are read, negative ones passed over; an index occurs at most
 * once per tree).
 *   out_rf           [T][T]  Robinson-Foulds distance |A| + |B| - 2 |A n B| over the NONTRIVIAL
 *                            splits (index >= n) of the two trees; symmetric, zero diagonal
 *   out_branch_score [T][T] or NULL: sum over the splits of either tree, trivial ones included,
 *                            of (l_a - l_b)^2, an absent split counting as length 0: the SQUARED
 *                            Kuhner-Felsenstein branch score.  Terms are added in ascending split
 *                            index, one accumulator, every operation rounded once: the result
 *                            depends neither on T nor on the pair's place in the launch.  Needs
 *                            branch_lengths.
 * At most 2049 taxa (a tree's sorted list is kept in LDS). */
int32_t mi_engine_rf_distances(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                               const int32_t* split_index /* [T][2n-1] */,
                               const double* branch_lengths /* [T][2n-2] or NULL */,
                               int32_t* out_rf /* [T][T] */, double* out_branch_score /* [T][T] or NULL */);

/* The majority-rule consensus tree of a split table (host arithmetic only, like
 * mi_nni_neighbour).  Every nontrivial split with split_weight > threshold * total_weight is
 * kept (split_weight: column 0 of the statistics, or the tree counts); threshold is in
 * [0.5, 1): below 0.5 is refused, because a strict majority is what makes the kept splits
 * pairwise compatible (kept splits that are not are an error).  The result is the tree they
 * form, in the reference's convention: leaves 0..n-1, internal nodes in post-order with the
 * children ordered by largest leaf id, the root last -- it holds leaf 0, the maximal kept sets
 * and the leaves none of them covers, so its degree is at least 3.
 *   out_node_count [1]    m, n+1 <= m <= 2n-2
 *   out_parent_ids [m-1]  (capacity 2n-3)
 *   out_node_split [m]    table index of each node's edge (-1: the root, or a leaf whose
 *                         trivial split the table lacks); capacity 2n-2
 * A fully resolved result (m = 2n-2) is a valid input to every unrooted call. */
int32_t mi_consensus_tree(int32_t taxon_count, int32_t split_count, const uint32_t* split_bits /* [S][W] */,
                          const double* split_weight /* [S] */, double total_weight, double threshold,
                          int32_t* out_node_count, int32_t* out_parent_ids, int32_t* out_node_split);

/* ---- subsplit Bayesian networks of unrooted trees (an extension) ----
 * What the reference's UnrootedSBNMaps (src/sbn_maps.cpp) and SBNProbability
 * (src/sbn_probability.cpp) compute on the host with bitset maps, for a batch of trees on the
 * device.  Trees have the form every unrooted call takes: n taxa, E = 2n-3 edges, edge v the
 * branch above node v, the root 2n-3 of degree 3.  The split table (above) names every clade by
 * an integer, 2 split + side: side 0 is the stored split (never taxon 0), side 1 its complement.
 *
 * Directed edge d = 2v + s.  s = 0: the focal clade is the leaf set below v, the far node is
 * parent(v), the focal node is v.  s = 1: the focal clade is everything else, the far node is v,
 * the focal node is parent(v) and its two child clades are its other two neighbours'.
 * Slot (d, k), k in {0, 1, 2}: it exists only if the focal clade has at least 2 taxa.
 *   k = 0     the sister is the complement of the focal clade (the rooting on that very edge)
 *   k = 1, 2  the sister is one of the far node's other two clades (far node internal only):
 *             s = 0, parent(v) not the root: the sibling's clade, then the clade above parent(v);
 *             s = 0 under the root: the two siblings in ascending node id;
 *             s = 1: v's two children in ascending node id.
 * The slot's PCSP is (sister | focal | child), the child being the one of the focal node's two
 * child clades that does NOT hold the focal clade's lowest-numbered taxon (what std::min over the
 * reference's bitsets picks, src/sbn_maps.cpp:78).  A tree has at most 6 (2n-3) slots; the
 * reference's per-rooting lists (O(n^2) per tree) are never formed on the device.
 *
 * Parameters: a vector of length P = S + C.  Entries 0 .. S-1 are the rootsplits: every split of
 * the support, with the split table's indices.  Entries S .. P-1 are the C distinct PCSPs in
 * contiguous blocks per parent (sister | focal); blocks are ordered by the first occurrence of the
 * parent in (tree, d, k) order, children within a block by their own first occurrence.  (The
 * reference's numbering follows the iteration order of an unordered_map: it is not reproduced.)
 * The support is that of trees 0 .. support_tree_count-1; the later trees are only looked up, and
 * a rootsplit or PCSP they alone hold gets the sentinel P (the reference's out_of_sample_index).
 *
 * The rooting on edge v has  log p_v = theta[root(v)] + A(2v, 0) + A(2v+1, 0),
 *   A(d, k) = theta[slot(d, k)] + B(d),  B(d) = sum over the two child directed edges c of d whose
 *   focal clade is no leaf of A(c, k_c), k_c the slot of c whose sister is c's sibling
 * (A = 0 for a leaf clade), and log q = logsumexp_v log p_v.  Orders of the sums: B adds the lower
 * child (s = 0), resp. the sibling before the edge above or the lower sibling under the root
 * (s = 1), first; log p_v adds from left to right as written; log q takes the maximum m, adds
 * exp(log p_v - m) in ascending v and adds log of the sum to m.  A rooting that touches the
 * sentinel or a -inf parameter has log p_v = -inf; a tree without a rooting in the support has
 * log q = -inf.  There is no NaN.
 *
 * mi_engine_sbn_index: the support and every tree's slots.  Any engine serves.
 *   out_root_index [T][2n-3]          parameter index of the rootsplit of edge v, or P
 *   out_slot_index [T][2(2n-3)][3]    -1: no such slot; P: outside the support; else the index
 *   out_counts [3]                    S, C, and the number of parents (blocks)
 *   out_split_bits [rootsplit_capacity][W]  the rootsplits, as mi_engine_split_index stores them
 *   out_pcsp_clades [pcsp_capacity][3]      sister, focal, child of PCSP S + i, each 2 split + side
 *   out_parent_range [pcsp_capacity][2]     parameter range [begin, end) of block b
 *   out_pcsp_parent [pcsp_capacity]         the block of PCSP S + i
 * Rows at and above the counts stay untouched.  S > rootsplit_capacity or C > pcsp_capacity is an
 * error whose message carries both counts (T0 (2n-3) and 6 T0 (2n-3) always suffice).  A refused
 * tree is named as by mi_engine_split_index.  The call is not chunked: a batch whose workspace is
 * over the arena budget (MI_PHYLO_PLV_BYTES) is refused with the sizes in the message.
 * mi_engine_last_call_path of every SBN call: "sbn n=<n> store=lds|global". */
int32_t mi_engine_sbn_index(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                            const int32_t* parent_ids /* [T][2n-3] */, int32_t support_tree_count,
                            int32_t rootsplit_capacity, int32_t pcsp_capacity,
                            int32_t* out_root_index, int32_t* out_slot_index, int32_t* out_counts,
                            uint32_t* out_split_bits, int32_t* out_pcsp_clades, int32_t* out_parent_range,
                            int32_t* out_pcsp_parent);

/* Probabilities of a batch under given parameters (SBNProbability::ProbabilityOfSingle in log
 * space, and the E-step).  log_params [P]: entries may be -inf; NaN and +inf are refused.
 * normalized = 0: the vector is log-normalised per block first (mi_engine_sbn_normalize).
 *   out_rooting_log_prob [T][2n-3]  log p_v
 *   out_log_q [T]
 *   out_log_expected_counts [P] or NULL: log sum_t w_t usage_t[j], w = tree_weights (NULL: 1;
 *       finite and >= 0).  usage: rho_v = exp(log p_v - log q) for the rootsplit of v and both
 *       k = 0 slots of v; a slot (d, k != 0) whose sister lies toward neighbour w of the far node
 *       x is used by the rootings on the edges beyond x's third neighbour u, the edge (x, u)
 *       included.  These region sums are formed in log space, one ascending and one descending
 *       pass: R(d) = log(exp(log rho of d's edge) + exp(R(c1)) + exp(R(c2))) over the child
 *       directed edges in the order of B above.  Over the trees, a parameter's terms are added in
 *       ascending (tree, entry) order, entry = edge for a rootsplit, else 2n-3 + 3 d + k: the
 *       maximum m of the terms, then sum exp(x - m), then m + log.  A parameter no tree uses, and
 *       a tree with log q = -inf, give -inf resp. add nothing.
 * This is the E-step and the building block of the gradient with respect to unnormalised
 * parameters phi (theta = log softmax per block): with G_j = sum_t w_t usage_t[j] and w_t the
 * coefficients of sum_t w_t log q_t,  d/d phi_j = G_j - exp(theta_j) sum_{i in block(j)} G_i.
 * Per-tree outputs depend on the tree alone: the same bits alone and inside any batch. */
int32_t mi_engine_sbn_log_prob(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                               const int32_t* parent_ids, const int32_t* root_index, const int32_t* slot_index,
                               int32_t rootsplit_count, int32_t pcsp_count, int32_t parent_count,
                               const int32_t* parent_range /* [parent_count][2] */,
                               const double* log_params /* [P] */, int32_t normalized,
                               const double* tree_weights /* [T] or NULL */, double* out_rooting_log_prob,
                               double* out_log_q, double* out_log_expected_counts /* [P] or NULL */);

/* SBNProbability::ProbabilityNormalizeParamsInLog: out[j] = in[j] - logsumexp of j's block, the
 * rootsplits [0, S) and every parent's range.  A block of up to 16 entries: the maximum m, then
 * the sum of exp(x - m) in ascending order.  A longer block is a wave's: lane l takes the maximum,
 * then the sum of exp(x - m), of entries l, l + 64, ..., and the lanes meet in a butterfly (offsets
 * 32, 16, .., 1).  A block that is all -inf stays -inf.  In place is allowed. */
int32_t mi_engine_sbn_normalize(mi_engine* engine, int32_t rootsplit_count, int32_t pcsp_count,
                                int32_t parent_count, const int32_t* parent_range, const double* log_params,
                                double* out_log_params);

/* Training on the batch (every tree must be in the support: a sentinel in a tree is an error that
 * names the tree).  tree_weights: the topology counts (NULL: 1); a duplicate tree in the batch is
 * the same as a larger weight, by linearity.
 *   MI_SBN_SA  SimpleAverage: the log of the weighted rooting counts (the usage with rho = 1),
 *              normalised.
 *   MI_SBN_EM  ExpectationMaximization (src/sbn_probability.cpp:214-329) in its mathematics: start
 *              from m~ = counts / (2n-3), normalised; per iteration the E-step (log m-bar = the
 *              expected counts of mi_engine_sbn_log_prob), theta = normalise(log m-bar), with
 *              alpha > 0 normalise(logaddexp(log m-bar, log alpha + log m~)); the score is
 *              sum_t w_t log q_t (under the parameters BEFORE the update) plus, for alpha > 0,
 *              sum_j alpha m~_j theta_j; stop when |score - previous| / |previous| < score_epsilon;
 *              fail if that ratio falls below the reference's -1e-10.  The reference's replacement
 *              of a log probability by DOUBLE_MINIMUM after a floating-point exception
 *              (fetestexcept) is not reproduced: nothing here raises one.
 *   out_log_params [P]          normalised
 *   out_score_history [max_iter]  zero beyond out_iterations (EM; may be NULL for SA)
 *   out_iterations [1]          EM iterations run (0 for SA) */
enum { MI_SBN_SA = 0, MI_SBN_EM = 1 };
int32_t mi_engine_sbn_train(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                            const int32_t* parent_ids, const int32_t* root_index, const int32_t* slot_index,
                            int32_t rootsplit_count, int32_t pcsp_count, int32_t parent_count,
                            const int32_t* parent_range, const double* tree_weights /* [T] or NULL */,
                            int32_t method, double alpha, int32_t max_iter, double score_epsilon,
                            double* out_log_params, double* out_score_history, int32_t* out_iterations);

/* ---- sampling from an SBN and the gradient of the variational objective ----
 * What the reference's SampleTrees (src/generic_sbn_instance.hpp:320-366) and TopologyGradients
 * (src/unrooted_sbn_instance.cpp:128-198, src/generic_sbn_instance.hpp:398-431) do on the host.
 *
 * The descent table: every parameter j leads to two parent subsplits, which the sampler visits.
 *   out_descent [P][2]   >= 0: a block (an index into parent_range); < 0: the leaf ~value
 * Rootsplit j < S with the stored split s (never taxon 0): entry 0 is (focal s, sister ~s), entry 1
 * (focal ~s, sister s).  PCSP (sister | focal | child): entry 0 is (focal child, sister
 * focal \ child), entry 1 (focal focal \ child, sister child).  The pairs are taken from the
 * support trees' own slots: the PCSP of slot (d, k) leads to the slots (c, k_c) of d's two child
 * directed edges, k_c as in B(d) above; such a slot's entry is the block of its PCSP
 * (pcsp_parent), or ~taxon where c's focal clade is a leaf.  Every occurrence of a parameter
 * writes the same pair.  Only trees 0 .. support_tree_count-1 are read; a sentinel (or a refused
 * tree) among them is an error that names the tree. */
int32_t mi_engine_sbn_descent(mi_engine* engine, int32_t support_tree_count, int32_t taxon_count,
                              const int32_t* parent_ids, const int32_t* root_index, const int32_t* slot_index,
                              int32_t rootsplit_count, int32_t pcsp_count, const int32_t* pcsp_parent /* [C] */,
                              int32_t* out_descent /* [P][2] */);

/* sample_count topologies drawn from the SBN with parameters log_params [P] (unnormalised is fine;
 * -inf allowed; NaN and +inf refused).
 * The CDF, per block (the rootsplits [0, S) and every parent's range), m the block's maximum:
 *   cdf[j] = sum over i <= j of the block of exp(log_params[i] - m)
 * added in ascending order with one accumulator, whatever the block's length (a block of more than
 * 16 entries is a wave's, which takes 64 exponentials side by side and adds them lane after lane:
 * the same additions in the same order).  A -inf entry adds 0; a block that is all -inf has a CDF
 * of zeros.  The CDF is non-decreasing within a block, and it is all the draws read.
 * Random numbers: Philox4x32-10 (multipliers D2511F53, CD9E8D57; key increments 9E3779B9,
 * BB67AE85).  Draw i of sample t = first_sample + k: key (seed lo, seed hi), counter
 * (i, 0, t lo, t hi), u = ((w0 << 32 | w1) >> 11) 2^-53 from the first two output words.  A
 * sample's bits depend on (seed, t) alone.
 * A draw in block [b, e): x = u cdf[e-1] (one rounded product); the smallest j with cdf[j] > x; if
 * there is none, the smallest j with cdf[j] == cdf[e-1].  Draw 0 is the rootsplit; then the two
 * entries of the chosen parameter are descended depth first, entry 0's subtree before entry 1's;
 * every visit of a block takes one draw.  A visited block whose total is 0 is an error that names
 * the sample (its position k in the call) and the block; that sample's integer outputs are -1
 * and its log probability NaN.
 *   out_parent_ids [K][2n-3]   the sampled rooted tree, de-rooted as Node::Deroot does (the
 *       trifurcation goes to the root child that holds taxon n-1 unless that child is a leaf, then
 *       to the other one; the remaining root child becomes its third child) and numbered as every
 *       unrooted call expects (leaves 0..n-1, internal nodes in post-order, children by largest
 *       leaf id, the root 2n-3)
 *   out_root_edge [K]          the new id of that third child: the sampled rooting is on its edge
 *   out_sampled_params [K][n-1]  the drawn indices in the order of the draws
 *   out_log_prob [K]           sum over them, in that order, one accumulator, of
 *                              (log_params[j] - m_b) - log(cdf[e_b - 1])
 *   out_cdf [P] or NULL        the CDF the draws read */
int32_t mi_engine_sbn_sample(mi_engine* engine, int32_t sample_count, int32_t taxon_count,
                             int32_t rootsplit_count, int32_t pcsp_count, int32_t parent_count,
                             const int32_t* parent_range, const int32_t* descent /* [P][2] */,
                             const double* log_params /* [P] */, uint64_t seed, int64_t first_sample,
                             int32_t* out_parent_ids, int32_t* out_root_edge, int32_t* out_sampled_params,
                             double* out_log_prob, double* out_cdf);

/* The gradient of the multi-sample variational objective with respect to the unnormalised SBN
 * parameters: out_gradient[j] = G_j - exp(theta_j) sum_{i in block(j)} G_i (the block's sum in
 * ascending order), G_j = sum_t a_t usage_t[j] with the usage of mi_engine_sbn_log_prob.  Every
 * usage is taken to the linear domain per term (each in [0, 1]), multiplied by a_t, and a
 * parameter's terms are added signed in ascending (tree, entry) order with one accumulator.  A
 * tree with log q = -inf adds nothing (the reference gives NaN there) and sentinel entries are
 * skipped.  The factors a_t from log_f [K]:
 *   MI_SBN_FACTORS_PLAIN  log F = logsumexp(log_f) (the maximum, then ascending);
 *                         a_t = (log F - log K) - exp(log_f[t] - log F)
 *   MI_SBN_FACTORS_VIMCO  the plain factor minus the per-sample signal: logsumexp over the K values
 *                         with log_f[t] replaced by (sum log_f - log_f[t]) / (K - 1), minus log K;
 *                         a fresh logsumexp per t.  K < 2 is refused.
 *   MI_SBN_FACTORS_GIVEN  a_t = log_f[t]
 *   out_gradient [P], out_factors [K], out_log_q [K] */
enum { MI_SBN_FACTORS_PLAIN = 0, MI_SBN_FACTORS_VIMCO = 1, MI_SBN_FACTORS_GIVEN = 2 };
int32_t mi_engine_sbn_topology_gradient(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                                        const int32_t* parent_ids, const int32_t* root_index,
                                        const int32_t* slot_index, int32_t rootsplit_count, int32_t pcsp_count,
                                        int32_t parent_count, const int32_t* parent_range,
                                        const double* log_params, int32_t normalized, const double* log_f,
                                        int32_t estimator, double* out_gradient, double* out_factors,
                                        double* out_log_q);

/* ---- PSP indexing and the log-normal branch-length models (an extension) ----
 * The branch-length side of a variational step: every tree's edges are indexed by split or by
 * primary subsplit pair (PSP), every particle's branch lengths are drawn from a log-normal q whose
 * (mu, sigma) are sums over those indices, and the gradient with respect to the (mu, sigma) tables
 * comes by the reparametrisation trick (the reference's vip/branch_model.py and
 * vip/scalar_model.py).  Any engine serves, 4 or 20 states: the taxon count is an argument and
 * the alignment plays no part; a sharded handle lets its first shard do the work.  FP64
 * throughout, no floating-point atomics, every sum in the one order stated here.
 *
 * A PSP is a PCSP of the support whose sister is the complement of its focal clade:
 * pcsp_clades[i][0] == pcsp_clades[i][1] ^ 1 (the reference's PCSPIsRootsplit); its name is
 * "focal|child" (PCSPWithoutParent).  In a tree these are the k = 0 slots: the "up" PSP of edge v
 * is slot (2v+1, 0), the "down" PSP is slot (2v, 0) (absent for a pendant edge).
 *
 * mi_engine_psp_table: the PSP numbering of a support.
 *   out_psp_of_pcsp [C]  S + the rank of PCSP i among the PSPs in ascending parameter order, or -1
 *   out_counts [2]       S and V = S + the number of PSPs (the reference's first_empty_index)
 * The variables are 0 .. V-1: the rootsplits, then the PSPs.  The reference numbers its PSPs in the
 * iteration order of an unordered_map, which is not reproduced: the SETS of names agree. */
int32_t mi_engine_psp_table(mi_engine* engine, int32_t rootsplit_count, int32_t pcsp_count,
                            const int32_t* pcsp_clades /* [C][3] */, int32_t* out_psp_of_pcsp, int32_t* out_counts);

/* The index rows of trees that mi_engine_sbn_index has given their root_index and slot_index
 * (support trees or trees behind them): out_index [T][rows][2n-3], rows 1 (the split model) or 3.
 *   row 0  root_index[t][v]                          (the reference's rootsplit_position)
 *   row 1  psp_of_pcsp of slot (2v, 0)               (subsplit_down_position)
 *   row 2  psp_of_pcsp of slot (2v + 1, 0)           (subsplit_up_position)
 * Whatever is not a variable becomes variable_count (V): a slot that does not exist (-1), an entry
 * outside the support (P) and a rootsplit outside the support.  This is the reference's "not
 * present" index; the calls below skip it.  rows = 1 reads neither slot_index nor psp_of_pcsp. */
int32_t mi_engine_psp_index(mi_engine* engine, int32_t tree_count, int32_t taxon_count, const int32_t* root_index,
                            const int32_t* slot_index, int32_t rootsplit_count, int32_t pcsp_count,
                            const int32_t* psp_of_pcsp /* [C] */, int32_t variable_count, int32_t rows,
                            int32_t* out_index);

/* Branch lengths of tree_count particles drawn from the log-normal q, with log q and the
 * exponential prior.  index [T][rows][2n-3] (rows 1 or 3), q_params [V][2] = (mu, sigma) per
 * variable.  An index outside [0, V) is not a variable and adds nothing.  Per tree t and edge v:
 *   mu = 0 + q[index[t][0][v]][0] + q[index[t][1][v]][0] + ..., rows in ascending order; sigma
 *   likewise from q[.][1].  sigma <= 0 or not finite, or a NaN mu, is an error that names the tree
 *   and the edge (a row of sentinels alone gives sigma = 0).
 *   eps = epsilon_in[t][v] if epsilon_in is given (the reference's prebaked_sample; antithetic
 *   draws), else a standard normal from Philox4x32-10 (constants as mi_engine_sbn_sample): key
 *   (seed lo, seed hi), counter (v, 1, s lo, s hi), s = first_sample + t -- the second counter
 *   word is 1, so the stream is disjoint from mi_engine_sbn_sample's under the same seed;
 *   u1 = (((w0 << 32 | w1) >> 11) + 1) 2^-53 in (0, 1], u2 = ((w2 << 32 | w3) >> 11) 2^-53,
 *   eps = sqrt(-2 log u1) cos((2 pi) u2).  An edge's bits depend on (seed, s, v) alone.
 *   x = mu + sigma eps (a rounded product, a rounded sum), theta = exp(x).
 *   out_branch_lengths [T][2n-2]  theta; entry 2n-3 is 0: the layout the likelihood calls take
 *   out_epsilon [T][2n-3]
 *   out_log_q [T]     -sum_v (((x + log sigma) + log(2 pi)/2) + 0.5 (eps eps)), with x itself, the
 *                     terms added in ascending v with one accumulator from 0
 *   out_log_prior [T] (2n-3) log(prior_rate) - prior_rate sum_v theta, the sum in the same order
 * prior_rate must be finite and positive (the reference's is 10). */
int32_t mi_engine_branch_model_sample(mi_engine* engine, int32_t tree_count, int32_t taxon_count, int32_t rows,
                                      const int32_t* index, int32_t variable_count, const double* q_params,
                                      uint64_t seed, int64_t first_sample, double prior_rate,
                                      const double* epsilon_in /* [T][2n-3] or NULL */, double* out_branch_lengths,
                                      double* out_epsilon, double* out_log_q, double* out_log_prior);

/* The gradient of sum_t w_t (log p_t - log q_t) with respect to q_params by the reparametrisation
 * trick, and the log_f vector mi_engine_sbn_topology_gradient takes.  branch_lengths, epsilon,
 * log_q_branch and log_prior are the sample call's outputs for the same index and q_params;
 * branch_gradient [T][2n-1] and log_likelihoods [T] are mi_engine_gradients_unrooted's.
 * Per tree t and edge v, with d = branch_gradient[t][v] - prior_rate and w = tree_weights[t] (1 if
 * NULL), sigma as in the sample call (checked the same way):
 *   c0 = w ((d theta) + 1)
 *   c1 = w ((((d theta) eps) + eps) + (1 / sigma))
 * every operation rounded once, in the order the parentheses give.
 *   out_gradient [V][2]  row j: the sum of c0 resp. c1 over every entry (t, r, v) with
 *       index[t][r][v] == j, in ascending entry number of the [T][rows][2n-3] array, one
 *       accumulator per component from 0 (a run of more than 16 entries is a wave's, 64 entries
 *       side by side and added lane after lane: the same additions in the same order).  A variable
 *       no entry names gets 0.  This is SplitModel.scalar_grad for rows = 1 and what
 *       PSPModel.scalar_grad computes for every real variable for rows = 3 (its sentinel row, zero
 *       by decree, does not exist here).
 *   out_log_f [T]  ((beta log_likelihoods[t] + log_prior[t]) - log_q_topology[t]) - log_q_branch[t]
 *       (log_q_topology NULL: 0).  As in the reference, beta scales the likelihood in log_f only. */
int32_t mi_engine_branch_model_gradient(mi_engine* engine, int32_t tree_count, int32_t taxon_count, int32_t rows,
                                        const int32_t* index, int32_t variable_count, const double* q_params,
                                        const double* branch_lengths, const double* epsilon,
                                        const double* log_q_branch, const double* log_prior,
                                        const double* branch_gradient, const double* log_likelihoods,
                                        const double* log_q_topology /* [T] or NULL */,
                                        const double* tree_weights /* [T] or NULL */, double beta, double prior_rate,
                                        double* out_gradient, double* out_log_f);

/* Maximum-likelihood branch lengths of unrooted trees under box bounds (an extension: the
 * consumer of the Hessian call's outputs).  Every tree of the batch is
 * iterated on the device: an evaluation is one Hessian pass at a trial point, a step is a
 * safeguarded diagonal Newton step from g, H and S, accepted when the log-likelihood does
 * not fall by more than its rounding error (2^-48 |logL|).  A tree stops when max_j |pg_j| max(t_j, 1e-3) <= tolerance at its accepted point
 * (pg: the gradient, 0 where t_j sits on a bound and the gradient points outward), when its
 * step scale has fallen below 2^-20, or after max_iterations evaluations.
 *   out_branch_lengths  [T][2n-2]  the last accepted point (the entry of the fixed node, 2n-3,
 *                                  is the caller's, unchanged)
 *   out_log_likelihoods [T], out_branch_gradient / out_branch_hessian [T][2n-1] or NULL:
 *                                  the Hessian call's outputs at that point
 *   out_iterations      [T] or NULL: evaluations the tree used, the first one included
 *   out_status          [T]        MI_BRANCH_OPT_*
 * Returns 0 when it ran, whatever the per-tree statuses; nonzero for bad arguments and
 * per-tree input errors.  4-state engines only.  Sharded handles: MI_SHARD_TREES deals the
 * trees as the other calls do (each shard optimises its block; results in tree order);
 * MI_SHARD_PATTERNS is refused (every iteration would need a sum across the shards).
 * mi_engine_last_call_path names the Hessian kernel that ran and adds
 * "opt iters=<passes> evals=<tree evaluations> batches=<trees>x<passes>,..."; the evaluation
 * count of mi_engine_last_call_info is the number of tree evaluations done. */
enum { MI_BRANCH_OPT_CONVERGED = 0, MI_BRANCH_OPT_ITERATION_LIMIT = 1, MI_BRANCH_OPT_STALLED = 2 };
typedef struct {
  int32_t max_iterations; /* evaluations per tree, 1..1000 (default 100) */
  int32_t check_interval; /* passes between two reads of the active count (default 4) */
  int32_t pack_active;    /* 1: passes run on the active trees only (default); 0: on all T */
  double tolerance;       /* default 1e-6 */
  double min_length;      /* default 1e-8 */
  double max_length;      /* default 10 */
  int32_t reserved[4];    /* 0 */
} mi_branch_opt_options;
int32_t mi_engine_optimize_branch_lengths_unrooted(
    mi_engine* engine, int32_t tree_count, const int32_t* parent_ids /* [T][2n-3] */,
    const double* start_branch_lengths /* [T][2n-2] */, const double* params, int32_t rescaling,
    const mi_branch_opt_options* options /* NULL: the defaults */,
    double* out_branch_lengths /* [T][2n-2] */, double* out_log_likelihoods /* [T] */,
    double* out_branch_gradient /* [T][2n-1] or NULL */,
    double* out_branch_hessian /* [T][2n-1] or NULL */, int32_t* out_iterations /* [T] or NULL */,
    int32_t* out_status /* [T] */);

/* Taking NNI moves on the device (an extension): for every tree of the batch
 * the tree mi_nni_neighbour(n, parent_ids[t], branch_lengths[t], v, i, ...) returns for
 * moves[t] = 2 v + i (what out_best_move of the scan gives), bit for bit -- leaves keep their
 * ids, internal nodes in post-order with the children ordered by largest leaf id, every branch
 * length moved to its subtree's new id, the entry of 2n-3 copied -- or a copy of the tree for
 * moves[t] = -1.  A code that is neither -1 nor that of an inner edge (n <= v < 2n-3), or a
 * parent-id vector that is no tree in the reference's form, is a per-tree error ("... (tree
 * t)"); that tree's outputs are a copy of its inputs.  No output may overlap an input.  Any
 * engine serves (the alignment plays no part); a sharded handle lets its first shard do it. */
int32_t mi_engine_nni_apply_unrooted(mi_engine* engine, int32_t tree_count,
                                     const int32_t* parent_ids /* [T][2n-3] */,
                                     const double* branch_lengths /* [T][2n-2] */,
                                     const int32_t* moves /* [T]: 2 v + i, or -1: copy the tree */,
                                     int32_t* out_parent_ids /* [T][2n-3] */,
                                     double* out_branch_lengths /* [T][2n-2] */);

/* NNI hill climbing of unrooted trees on the device (an extension).  Per
 * tree, a round optimises the branch lengths by the rule of
 * mi_engine_optimize_branch_lengths_unrooted, unchanged, from the lengths the tree carries
 * (the caller's at first), and scans the neighbourhood (mi_engine_nni_scan_unrooted) at the
 * optimised lengths.  If the largest delta exceeds min_gain and the tree has taken fewer than
 * max_moves moves, it takes the scan's best move (the lowest code among equals), logs the code
 * -- in the ids of the tree AT THAT ROUND -- and its delta, and goes round again with the
 * lengths the move carries along.  Otherwise it stops: MI_NNI_SEARCH_LOCAL_OPTIMUM when no
 * delta exceeds min_gain, MI_NNI_SEARCH_MOVE_LIMIT otherwise.  A three-taxon tree stops after
 * one optimisation with 0 moves.
 *   out_parent_ids / out_branch_lengths  topology and lengths of the tree's LAST optimisation
 *   out_log_likelihoods   [T]       that optimisation's logL (the Hessian call's)
 *   out_best_delta        [T] or NULL: the largest delta of the scan there (0 when n == 3)
 *   out_move_count        [T]       moves taken
 *   out_move_log / out_move_gain  [T][max_moves] or NULL: code and delta of every move taken;
 *                                   unused entries are -1 and 0
 *   out_status            [T]       MI_NNI_SEARCH_*
 *   out_branch_opt_status [T] or NULL: MI_BRANCH_OPT_* of that optimisation
 * min_gain: the optimiser lets logL fall by at most 2^-48 |logL| per pass, and the scan's and
 * the Hessian call's logL agree to 1e-12 relative, so the default 1e-3 is about five orders
 * above both at |logL| = 1e4: every round's logL is then strictly above the last and no
 * topology can recur.  Below about 1e-8 |logL| that argument no longer holds (such values are
 * accepted): max_moves is then what ends the loop.
 * Every round runs on the trees that are still searching (pack_active), routed as the whole
 * batch would be, so a tree's numbers do not depend on which others are still searching.
 * Returns 0 when it ran, whatever the per-tree statuses; nonzero for bad arguments (max_moves,
 * min_gain, the optimiser's own checks) and per-tree input errors.  4-state engines only.
 * Sharded handles: MI_SHARD_TREES deals the trees as the other calls do (each shard searches
 * from its block, one after the other; results in tree order); MI_SHARD_PATTERNS is refused,
 * for the optimiser's reason.  mi_engine_last_call_path is the last Hessian pass's path plus
 * " nni-search rounds=<r> moves=<total> batches=<trees>x<rounds>,..."; the evaluation count of
 * mi_engine_last_call_info is the tree evaluations done: the optimiser's plus one per scan. */
enum { MI_NNI_SEARCH_LOCAL_OPTIMUM = 0, MI_NNI_SEARCH_MOVE_LIMIT = 1 };
typedef struct {
  int32_t max_moves;   /* moves per tree, 0..10000 (default 100); 0: optimise and scan only */
  int32_t pack_active; /* 1: rounds run on the trees still searching (default); 0: on all T */
  double min_gain;     /* a move is taken when its delta exceeds this; >= 0, default 1e-3 */
  int32_t reserved[4]; /* 0 */
  mi_branch_opt_options branch_opt; /* the optimiser's options for every round (zeros: its defaults) */
} mi_nni_search_options;
int32_t mi_engine_nni_search_unrooted(
    mi_engine* engine, int32_t tree_count, const int32_t* parent_ids /* [T][2n-3] */,
    const double* start_branch_lengths /* [T][2n-2] */, const double* params, int32_t rescaling,
    const mi_nni_search_options* options /* NULL: the defaults */,
    int32_t* out_parent_ids /* [T][2n-3] */, double* out_branch_lengths /* [T][2n-2] */,
    double* out_log_likelihoods /* [T] */, double* out_best_delta /* [T] or NULL */,
    int32_t* out_move_count /* [T] */, int32_t* out_move_log /* [T][max_moves] or NULL */,
    double* out_move_gain /* [T][max_moves] or NULL */, int32_t* out_status /* [T] */,
    int32_t* out_branch_opt_status /* [T] or NULL */);

/* Taking SPR moves on the device (an extension): for every tree of the batch
 * the tree mi_spr_neighbour(n, parent_ids[t], branch_lengths[t], s, dir, f, ...) returns for
 * moves[t] = (s, dir, f) (what out_best_move of mi_engine_spr_scan_unrooted gives), bit for bit
 * -- leaves keep their ids, internal nodes in post-order with the children ordered by largest
 * leaf id, the trifurcating root 2n-3, rooted at the caller's root if that node survives and at
 * the new attachment node otherwise, every length with its edge (along a reversed path too),
 * the merged edge the sum of the two doubles, the two halves 0.5 t_f, the entry of 2n-3 copied
 * -- or a copy of the tree for moves[t] = (-1, -1, -1).  Moves are triples, not packed codes:
 * (2 s + dir) (2n-3) + f leaves int32 for trees this call still takes.  A triple that
 * mi_spr_neighbour refuses (s or f out of range, dir neither 0 nor 1, dir = 1 on a leaf edge, f
 * in the moving part or a name of the merged edge), or a parent-id vector that is no tree in
 * the reference's form, is a per-tree error ("... (tree t)"); that tree's outputs are a copy of
 * its inputs and the engine stays usable.  No output may overlap an input.  Any engine serves
 * (the alignment plays no part); a sharded handle lets its first shard do it. */
int32_t mi_engine_spr_apply_unrooted(mi_engine* engine, int32_t tree_count,
                                     const int32_t* parent_ids /* [T][2n-3] */,
                                     const double* branch_lengths /* [T][2n-2] */,
                                     const int32_t* moves /* [T][3]: (s, dir, f), or (-1,-1,-1): copy the tree */,
                                     int32_t* out_parent_ids /* [T][2n-3] */,
                                     double* out_branch_lengths /* [T][2n-2] */);

/* SPR hill climbing of unrooted trees on the device (an extension): the
 * definition of mi_engine_nni_search_unrooted with the SPR scan in place of the NNI scan.  Per
 * tree, a round optimises the branch lengths by the rule of
 * mi_engine_optimize_branch_lengths_unrooted, unchanged, from the lengths the tree carries
 * (the caller's at first), and scans the neighbourhood (mi_engine_spr_scan_unrooted, within
 * `radius`) at the optimised lengths.  If the largest best_delta[s][dir] exceeds min_gain and
 * the tree has taken fewer than max_moves moves, it takes the scan's best_move (the lowest code
 * (2 s + dir) (2n-3) + f among equals), logs the triple -- in the ids of the tree AT THAT ROUND
 * -- and its delta, and goes round again with the lengths the move carries along (the merged
 * edge, the two halves, t_s).  Otherwise it stops: MI_SPR_SEARCH_LOCAL_OPTIMUM when no delta
 * exceeds min_gain, MI_SPR_SEARCH_MOVE_LIMIT otherwise.  A three-taxon tree stops after one
 * optimisation with 0 moves.
 *   out_parent_ids / out_branch_lengths  topology and lengths of the tree's LAST optimisation
 *   out_log_likelihoods   [T]       that optimisation's logL (the Hessian call's)
 *   out_best_delta        [T] or NULL: the largest delta of the scan there (0 when n == 3)
 *   out_move_count        [T]       moves taken
 *   out_move_log          [T][max_moves][3] or NULL: the triple of every move taken; unused: -1
 *   out_move_gain         [T][max_moves] or NULL: its delta; unused entries are 0
 *   out_status            [T]       MI_SPR_SEARCH_*
 *   out_branch_opt_status [T] or NULL: MI_BRANCH_OPT_* of that optimisation
 * min_gain and termination: the neighbour enters the next optimisation at logL + delta (the
 * scan's delta is formed per pattern, against the same tree's L_p), and the optimiser lets logL
 * fall by at most 2^-48 |logL| per pass, so with the default 1e-3 -- about five orders above
 * that at |logL| = 1e4 -- every round's logL is strictly above the last and no topology can
 * recur.  Below about 1e-8 |logL| that argument no longer holds (such values are accepted):
 * max_moves is then what ends the loop.
 * Every round runs on the trees that are still searching (pack_active), routed as the whole
 * batch would be, so a tree's numbers do not depend on which others are still searching.  The
 * scan's workspace is large; a batch over MI_PHYLO_PLV_BYTES is cut into
 * launches by the scan itself.
 * Returns 0 when it ran, whatever the per-tree statuses; nonzero for bad arguments (max_moves,
 * min_gain, a negative radius -- refused before any device work --, the optimiser's own checks)
 * and per-tree input errors.  4-state engines only.  Sharded handles: MI_SHARD_TREES deals the
 * trees as the other calls do (each shard searches from its block, one after the other; results
 * in tree order); MI_SHARD_PATTERNS is refused, for the optimiser's reason.
 * mi_engine_last_call_path is the last Hessian pass's path plus
 * " spr-search radius=<r> rounds=<r> moves=<total> batches=<trees>x<rounds>,..."; the
 * evaluation count of mi_engine_last_call_info is the tree evaluations done: the optimiser's
 * plus one per scan. */
enum { MI_SPR_SEARCH_LOCAL_OPTIMUM = 0, MI_SPR_SEARCH_MOVE_LIMIT = 1 };
typedef struct {
  int32_t max_moves;   /* moves per tree, 0..10000 (default 100); 0: optimise and scan only */
  int32_t pack_active; /* 1: rounds run on the trees still searching (default); 0: on all T */
  double min_gain;     /* a move is taken when its delta exceeds this; >= 0, default 1e-3 */
  int32_t radius;      /* the scan's: 0 (default) every move, >= 1 moves of distance <= radius */
  int32_t reserved[3]; /* 0 */
  mi_branch_opt_options branch_opt; /* the optimiser's options for every round (zeros: its defaults) */
} mi_spr_search_options;
int32_t mi_engine_spr_search_unrooted(
    mi_engine* engine, int32_t tree_count, const int32_t* parent_ids /* [T][2n-3] */,
    const double* start_branch_lengths /* [T][2n-2] */, const double* params, int32_t rescaling,
    const mi_spr_search_options* options /* NULL: the defaults */,
    int32_t* out_parent_ids /* [T][2n-3] */, double* out_branch_lengths /* [T][2n-2] */,
    double* out_log_likelihoods /* [T] */, double* out_best_delta /* [T] or NULL */,
    int32_t* out_move_count /* [T] */, int32_t* out_move_log /* [T][max_moves][3] or NULL */,
    double* out_move_gain /* [T][max_moves] or NULL */, int32_t* out_status /* [T] */,
    int32_t* out_branch_opt_status /* [T] or NULL */);

/* Engine::LogLikelihoods(const RootedTreeCollection&) when with_jacobian != 0
 * (branch lengths x rates, + log-det-Jacobian, fat_beagle.cpp:82-104), or
 * Engine::UnrootedLogLikelihoods(const RootedTreeCollection&) when 0
 * (fat_beagle.cpp:78-80: raw branch lengths, no Jacobian; rates/heights/bounds
 * may then be NULL). */
int32_t mi_engine_log_likelihoods_rooted(mi_engine* engine, int32_t tree_count,
                                         const int32_t* parent_ids,    /* [T][2n-2] */
                                         const double* branch_lengths, /* [T][2n-1] */
                                         const double* params,
                                         const double* rates,        /* [T][2n-2] RootedTree::rates_ */
                                         const double* node_heights, /* [T][2n-1] */
                                         const double* node_bounds,  /* [T][2n-1] */
                                         int32_t with_jacobian, int32_t rescaling,
                                         double* out_log_likelihoods);

/* Engine::Gradients(const RootedTreeCollection&, ...).
 * out_log_likelihoods excludes the Jacobian (rooted_sbn_instance.hpp:285).
 * out_ratios_root_height[T][n-1], out_clock_gradient[T][2n-2] (strict clock,
 * rate_counts[t]==1: entry 0 holds the single value, rest 0; per-branch clock,
 * rate_counts[t]==2n-2: all entries; anything else is an error,
 * fat_beagle.cpp:375-386). */
int32_t mi_engine_gradients_rooted(mi_engine* engine, int32_t tree_count,
                                   const int32_t* parent_ids, const double* branch_lengths,
                                   const double* params, const double* rates,
                                   const int32_t* rate_counts, /* [T] */
                                   const double* node_heights, const double* node_bounds,
                                   const double* height_ratios, /* [T][n-1] */
                                   int32_t rescaling, double* out_log_likelihoods,
                                   double* out_ratios_root_height, double* out_clock_gradient,
                                   double* out_site_gradient, double* out_subst_gradient);

/* ---- device-pointer entry points (asynchronous) -------------------------- */
/* Same arguments and meaning, but every array pointer is a device pointer on
 * the engine's device and nothing is synchronised: the work is enqueued on
 * `stream`.  Per-tree input errors (malformed parent ids, GTR sums off by
 * >= 1e-3, bad rate_count) set a device-side status word that
 * mi_engine_check_status() reads back (it synchronises the stream).
 *
 * A call never fails spuriously (the reference's Engine does not: src/engine.cpp:54-92).  A
 * gradient call of up to 512 small trees runs tree set-up and walk as ONE launch whose walk
 * waves wait -- bounded: one second of wall clock -- for their tree's set-up waves.  Should
 * that wait ever run out, the HOST-pointer entry points above run the call again at once
 * through the four-launch sequence and return those results (mi_engine_last_call_path then
 * says "setup=own-launch", and the engine keeps four launches from then on); a caller of the
 * *_device entry points finds the message at mi_engine_check_status and repeats the call --
 * a hipGraph captured before that still holds the one-launch kernel and must be captured
 * again.  (MI_PHYLO_FUSED_SETUP=0 selects four launches from the start.) */

int32_t mi_engine_log_likelihoods_unrooted_device(mi_engine* engine, void* stream,
                                                  int32_t tree_count, const int32_t* parent_ids,
                                                  const double* branch_lengths,
                                                  const double* params, int32_t rescaling,
                                                  double* out_log_likelihoods);
int32_t mi_engine_gradients_unrooted_device(mi_engine* engine, void* stream, int32_t tree_count,
                                            const int32_t* parent_ids,
                                            const double* branch_lengths, const double* params,
                                            int32_t rescaling, double* out_log_likelihoods,
                                            double* out_branch_gradient,
                                            double* out_site_gradient,
                                            double* out_subst_gradient);
int32_t mi_engine_log_likelihoods_rooted_device(mi_engine* engine, void* stream,
                                                int32_t tree_count, const int32_t* parent_ids,
                                                const double* branch_lengths,
                                                const double* params, const double* rates,
                                                const double* node_heights,
                                                const double* node_bounds,
                                                int32_t with_jacobian, int32_t rescaling,
                                                double* out_log_likelihoods);
int32_t mi_engine_gradients_rooted_device(mi_engine* engine, void* stream, int32_t tree_count,
                                          const int32_t* parent_ids,
                                          const double* branch_lengths, const double* params,
                                          const double* rates, const int32_t* rate_counts,
                                          const double* node_heights, const double* node_bounds,
                                          const double* height_ratios, int32_t rescaling,
                                          double* out_log_likelihoods,
                                          double* out_ratios_root_height,
                                          double* out_clock_gradient, double* out_site_gradient,
                                          double* out_subst_gradient);

int32_t mi_engine_gradients_unrooted_reduced_device(
    mi_engine* engine, void* stream, int32_t tree_count, const int32_t* parent_ids,
    const double* branch_lengths, const double* params, int32_t rescaling,
    const int32_t* branch_index, const double* tree_weights, int32_t index_count,
    double* out_sums, double* out_index_gradient, double* out_log_likelihoods);

int32_t mi_engine_branch_hessian_unrooted_device(mi_engine* engine, void* stream,
                                                 int32_t tree_count, const int32_t* parent_ids,
                                                 const double* branch_lengths,
                                                 const double* params, int32_t rescaling,
                                                 double* out_log_likelihoods,
                                                 double* out_branch_gradient,
                                                 double* out_branch_hessian,
                                                 double* out_branch_gradient_sq);

int32_t mi_engine_nni_scan_unrooted_device(mi_engine* engine, void* stream, int32_t tree_count,
                                           const int32_t* parent_ids, const double* branch_lengths,
                                           const double* params, int32_t rescaling,
                                           double* out_log_likelihoods, double* out_nni_delta,
                                           int32_t* out_best_move);

/* The device form of mi_engine_ancestral_states_unrooted: it only enqueues -- no allocation
 * and no synchronisation after mi_engine_reserve_ancestral(engine, tree_count), so it can be
 * captured in a hipGraph.  Output addresses are multiples of 16 bytes. */
int32_t mi_engine_ancestral_states_unrooted_device(
    mi_engine* engine, void* stream, int32_t tree_count, const int32_t* parent_ids,
    const double* branch_lengths, const double* params, int32_t rescaling, double* out_log_likelihoods,
    double* out_state_posteriors, int8_t* out_map_state, double* out_category_posteriors,
    double* out_pattern_rate, double* out_tip_posteriors);

/* The device form of mi_engine_placement_unrooted: every array a device pointer (the pendant
 * lengths too); it only enqueues -- no allocation and no synchronisation after
 * mi_engine_reserve_placement, so it can be captured in a hipGraph.  A column_pattern entry
 * outside [0, P) or a bad pendant length is reported through the status word
 * (mi_engine_check_status); the scoring clamps such an entry and reads nothing out of bounds. */
int32_t mi_engine_placement_unrooted_device(
    mi_engine* engine, void* stream, int32_t tree_count, const int32_t* parent_ids,
    const double* branch_lengths, const double* params, int32_t rescaling, int32_t query_count,
    int32_t column_count, const int8_t* query_states, const int32_t* column_pattern,
    const double* column_weights, int32_t pendant_count, const double* pendant_lengths,
    double* out_log_likelihoods, double* out_edge_log_likelihoods, int8_t* out_pendant_index,
    int32_t* out_best_edge, double* out_lwr, double* out_edge_tables);

/* The device form of mi_engine_spr_scan_unrooted: every array a device pointer; it only enqueues
 * -- no allocation and no synchronisation after mi_engine_reserve_spr_scan, so it can be captured
 * in a hipGraph.  A parent-id vector that is no tree is reported through the status word
 * (mi_engine_check_status); such a tree's rows hold no move. */
int32_t mi_engine_spr_scan_unrooted_device(mi_engine* engine, void* stream, int32_t tree_count,
                                           const int32_t* parent_ids, const double* branch_lengths,
                                           const double* params, int32_t rescaling, int32_t radius,
                                           double* out_log_likelihoods, int32_t* out_best_target,
                                           double* out_best_delta, int32_t* out_best_move, double* out_delta);

/* The device forms of mi_engine_pattern_log_likelihoods_unrooted, mi_engine_rell and
 * mi_engine_pattern_mixture: they only enqueue -- no allocation and no synchronisation after
 * mi_engine_reserve(tree_count, 0), mi_engine_reserve_rell and (the mixture) a first call of
 * that pattern count. */
int32_t mi_engine_pattern_log_likelihoods_unrooted_device(
    mi_engine* engine, void* stream, int32_t tree_count, const int32_t* parent_ids,
    const double* branch_lengths, const double* params, int32_t rescaling,
    double* out_log_likelihoods, double* out_pattern_log_likelihoods);
int32_t mi_engine_rell_device(mi_engine* engine, void* stream, int32_t replicate_count,
                              int32_t tree_count, int32_t pattern_count,
                              const double* pattern_log_likelihoods, const double* replicate_weights,
                              double* out_replicate_log_likelihoods, int32_t* out_best_tree,
                              double* out_bootstrap_proportion,
                              double* out_expected_likelihood_weight);
int32_t mi_engine_pattern_mixture_device(mi_engine* engine, void* stream, int32_t tree_count,
                                         int32_t pattern_count, const double* pattern_log_likelihoods,
                                         const double* tree_log_weights, const double* pattern_weights,
                                         double* out_pattern_log_marginal, double* out_log_marginal);

/* The device forms of mi_engine_bootstrap_weights and mi_engine_topology_tests (sites and
 * replicates stay host arrays: they fix the launch shapes and are read while the call enqueues):
 * they only enqueue -- no allocation and no synchronisation after
 * mi_engine_reserve_bootstrap_weights(B, P) / mi_engine_reserve_topology_tests(T, P, max_k
 * replicates[k]) --, and can be captured in a hipGraph.  What the host forms refuse about the
 * weights (no integer site counts, N outside [1, 2^31), sites[0] != N) goes to the status word
 * (mi_engine_check_status); the replicate weights of such a call are zeros. */
int32_t mi_engine_bootstrap_weights_device(mi_engine* engine, void* stream, int32_t pattern_count,
                                           const double* pattern_weights, int32_t replicate_count,
                                           int64_t sites, uint64_t seed, int64_t first_replicate,
                                           double* out_replicate_weights);
int32_t mi_engine_reserve_bootstrap_weights(mi_engine* engine, int32_t replicate_count, int32_t pattern_count);
int32_t mi_engine_topology_tests_device(mi_engine* engine, void* stream, int32_t tree_count,
                                        int32_t pattern_count, const double* pattern_log_likelihoods,
                                        const double* pattern_weights, int32_t block_count,
                                        const int64_t* sites, const int32_t* replicates, uint64_t seed,
                                        int64_t first_replicate, double* out_table, int32_t* out_counts,
                                        double* out_mean, double* out_replicate_log_likelihoods,
                                        int32_t* out_best_tree);
int32_t mi_engine_reserve_topology_tests(mi_engine* engine, int32_t tree_count, int32_t pattern_count,
                                         int32_t max_replicate_count);

/* The device form of mi_engine_optimize_branch_lengths_unrooted.  Unlike the other *_device
 * calls it SYNCHRONISES `stream` at its check points (it reads the number of active trees to
 * decide whether to go on), so it cannot be captured in a hipGraph; when it returns, every
 * kernel it needed has been enqueued, and the outputs are complete once the stream is. */
int32_t mi_engine_optimize_branch_lengths_unrooted_device(
    mi_engine* engine, void* stream, int32_t tree_count, const int32_t* parent_ids,
    const double* start_branch_lengths, const double* params, int32_t rescaling,
    const mi_branch_opt_options* options, double* out_branch_lengths, double* out_log_likelihoods,
    double* out_branch_gradient, double* out_branch_hessian, int32_t* out_iterations,
    int32_t* out_status);

/* The device form of mi_engine_nni_apply_unrooted: asynchronous, allocation-free after its
 * first call of that size (or mi_engine_reserve_nni_search), capturable in a hipGraph like the
 * other *_device calls; per-tree errors go to the status word (mi_engine_check_status). */
int32_t mi_engine_nni_apply_unrooted_device(mi_engine* engine, void* stream, int32_t tree_count,
                                            const int32_t* parent_ids, const double* branch_lengths,
                                            const int32_t* moves, int32_t* out_parent_ids,
                                            double* out_branch_lengths);
/* The device form of mi_engine_nni_search_unrooted.  Like the optimiser's it SYNCHRONISES
 * `stream` -- the optimiser at its check points, the search once per round, to read the number
 * of trees that moved -- so it cannot be captured in a hipGraph; when it returns, every kernel
 * it needed has been enqueued, and the outputs are complete once the stream is. */
int32_t mi_engine_nni_search_unrooted_device(
    mi_engine* engine, void* stream, int32_t tree_count, const int32_t* parent_ids,
    const double* start_branch_lengths, const double* params, int32_t rescaling,
    const mi_nni_search_options* options, int32_t* out_parent_ids, double* out_branch_lengths,
    double* out_log_likelihoods, double* out_best_delta, int32_t* out_move_count,
    int32_t* out_move_log, double* out_move_gain, int32_t* out_status,
    int32_t* out_branch_opt_status);
/* The device form of mi_engine_spr_apply_unrooted: asynchronous, allocation-free after its
 * first call of that size (or mi_engine_reserve_spr_search), capturable in a hipGraph like the
 * other *_device calls; per-tree errors go to the status word (mi_engine_check_status). */
int32_t mi_engine_spr_apply_unrooted_device(mi_engine* engine, void* stream, int32_t tree_count,
                                            const int32_t* parent_ids, const double* branch_lengths,
                                            const int32_t* moves, int32_t* out_parent_ids,
                                            double* out_branch_lengths);
/* The device form of mi_engine_spr_search_unrooted.  Like the optimiser's it SYNCHRONISES
 * `stream` -- the optimiser at its check points, the search once per round, to read the number
 * of trees that moved -- so it cannot be captured in a hipGraph; when it returns, every kernel
 * it needed has been enqueued, and the outputs are complete once the stream is.  It allocates
 * nothing after mi_engine_reserve_spr_search. */
int32_t mi_engine_spr_search_unrooted_device(
    mi_engine* engine, void* stream, int32_t tree_count, const int32_t* parent_ids,
    const double* start_branch_lengths, const double* params, int32_t rescaling,
    const mi_spr_search_options* options, int32_t* out_parent_ids, double* out_branch_lengths,
    double* out_log_likelihoods, double* out_best_delta, int32_t* out_move_count,
    int32_t* out_move_log, double* out_move_gain, int32_t* out_status,
    int32_t* out_branch_opt_status);

/* Make sure the workspace for `tree_count` trees exists (so that a following
 * *_device call allocates nothing and can be captured in a hipGraph).  20-state engines: if
 * the device cannot give the partial-vector arena its budget (MI_PHYLO_PLV_BYTES), the budget
 * is reduced and every buffer that scales with it is released and allocated again
 * (mi_engine_last_call_launches counts these back-offs) -- which invalidates graphs captured
 * on this engine BEFORE that: capture after the reservation, and again after any call that
 * reports a new back-off.  The fused-reduction entry points additionally need a sort
 * workspace that depends on index_count; it is allocated by their first call. */
int32_t mi_engine_reserve(mi_engine* engine, int32_t tree_count, int32_t for_gradients);
/* The same, plus the per-tree buffers and the index sort's workspace of
 * mi_engine_gradients_unrooted_reduced[_device] for up to `index_count` indices: a reduced
 * *_device call of at most that size then allocates nothing either (it used to
 * size and allocate its sort workspace inside the call). */
int32_t mi_engine_reserve_reduced(mi_engine* engine, int32_t tree_count, int32_t index_count);
/* The workspace of mi_engine_branch_hessian_unrooted[_device] for `tree_count` trees: a
 * *_device call of at most that size then allocates nothing (hipGraph capture).  4-state
 * engines only. */
int32_t mi_engine_reserve_hessian(mi_engine* engine, int32_t tree_count);
/* The workspace of mi_engine_nni_scan_unrooted[_device] for `tree_count` trees: a *_device
 * call of at most that size then allocates nothing (hipGraph capture).  4-state engines only. */
int32_t mi_engine_reserve_nni_scan(mi_engine* engine, int32_t tree_count);
/* The workspace of mi_engine_ancestral_states_unrooted[_device] for `tree_count` trees, of
 * either rescaling setting: a *_device call of at most that size then allocates nothing
 * (hipGraph capture).  4-state engines only. */
int32_t mi_engine_reserve_ancestral(mi_engine* engine, int32_t tree_count);
/* The workspace of mi_engine_spr_scan_unrooted[_device] for `tree_count` trees, of either
 * rescaling setting and any radius: a *_device call of at most that size then allocates nothing
 * (hipGraph capture).  4-state engines only. */
int32_t mi_engine_reserve_spr_scan(mi_engine* engine, int32_t tree_count);
/* The workspace of mi_engine_placement_unrooted[_device] for `tree_count` trees and
 * `pendant_count` pendant lengths, of either rescaling setting: a *_device call of at most that
 * size then allocates nothing (hipGraph capture).  query_count and column_count are checked;
 * the workspace does not depend on them.  4-state engines only. */
int32_t mi_engine_reserve_placement(mi_engine* engine, int32_t tree_count, int32_t query_count,
                                    int32_t column_count, int32_t pendant_count);
/* The workspace of mi_engine_optimize_branch_lengths_unrooted[_device] for `tree_count` trees
 * (the Hessian call's included): a *_device call of at most that size then allocates
 * nothing.  4-state engines only. */
int32_t mi_engine_reserve_branch_opt(mi_engine* engine, int32_t tree_count);
/* The workspace of mi_engine_nni_search_unrooted[_device] and of
 * mi_engine_nni_apply_unrooted[_device] for `tree_count` trees (the optimiser's and the scan's
 * included): a *_device call of at most that size then allocates nothing.  4-state engines
 * only. */
int32_t mi_engine_reserve_nni_search(mi_engine* engine, int32_t tree_count);
/* The workspace of mi_engine_spr_search_unrooted[_device] and of
 * mi_engine_spr_apply_unrooted[_device] for `tree_count` trees (the optimiser's and the SPR
 * scan's included): a *_device call of at most that size then allocates nothing.  4-state
 * engines only. */
int32_t mi_engine_reserve_spr_search(mi_engine* engine, int32_t tree_count);
/* The workspace of mi_engine_rell[_device] for `replicate_count` replicates and `tree_count`
 * trees (the [B][T] product when the caller wants none, the row statistics, the counts): a
 * *_device call of at most that size then allocates nothing.  `pattern_count` needs none. */
int32_t mi_engine_reserve_rell(mi_engine* engine, int32_t replicate_count, int32_t tree_count,
                               int32_t pattern_count);
/* The device forms of mi_engine_pairwise_distances, mi_engine_neighbour_joining and
 * mi_engine_starting_trees_unrooted: every array a device pointer (the options stay a host
 * struct).  They only enqueue; after mi_engine_reserve_start_trees they allocate nothing and
 * synchronise nothing, so they can be captured in a hipGraph: the iteration counts inside the
 * kernels are bounded by max_iterations and n, nothing is read back.  Per-call input errors (a
 * distance that is not finite, GTR parameters that do not sum to 1) go to the status word
 * (mi_engine_check_status). */
int32_t mi_engine_pairwise_distances_device(mi_engine* engine, void* stream, int32_t replicate_count,
                                            const double* replicate_weights, const double* params,
                                            const mi_distance_options* options, double* out_distances,
                                            double* out_pair_counts, int8_t* out_pair_status);
int32_t mi_engine_neighbour_joining_device(mi_engine* engine, void* stream, int32_t replicate_count,
                                           int32_t taxon_count, const double* distances,
                                           double min_length, double max_length,
                                           int32_t* out_parent_ids, double* out_branch_lengths);
int32_t mi_engine_starting_trees_unrooted_device(mi_engine* engine, void* stream,
                                                 int32_t replicate_count,
                                                 const double* replicate_weights, const double* params,
                                                 const mi_distance_options* options,
                                                 int32_t* out_parent_ids, double* out_branch_lengths,
                                                 double* out_distances);
/* The workspace of the three calls above for `replicate_count` replicates of the engine's own
 * alignment and taxon count (the tip codes, the model instance, the count workspace of a
 * chunk, the distances nobody asked for, neighbour joining's working sets).  It covers the
 * engine's OWN taxon count only: mi_engine_neighbour_joining_device with another taxon_count
 * allocates its workspace (beyond 128 taxa) and opts its kernel into large LDS at its first
 * call of that size -- run one such call before capturing it in a graph.  (Engines of several
 * hundred taxa: the set-up kernel that instantiates the model opts into large LDS at ITS first
 * launch, as in every other call -- there too, one call before the capture.)  4-state engines
 * only; a sharded handle reserves on its first shard. */
int32_t mi_engine_reserve_start_trees(mi_engine* engine, int32_t replicate_count);
/* The device forms of mi_engine_split_index and mi_engine_rf_distances: every array a device
 * pointer.  They only enqueue; after mi_engine_reserve_splits(engine, tree_count, taxon_count)
 * a call of at most that many trees of that taxon count allocates nothing and synchronises
 * nothing, so it can be captured in a hipGraph.  Input errors of a tree and a table larger than
 * split_capacity (whose rows at and above the capacity are then not written; *out_split_count
 * holds S) go to the status word (mi_engine_check_status).  A sharded handle reserves on its
 * first shard. */
int32_t mi_engine_split_index_device(mi_engine* engine, void* stream, int32_t tree_count, int32_t taxon_count,
                                     const int32_t* parent_ids, const double* branch_lengths,
                                     const double* tree_weights, int32_t split_capacity,
                                     int32_t* out_split_index, int32_t* out_split_count,
                                     uint32_t* out_split_bits, int32_t* out_split_first,
                                     int32_t* out_split_trees, double* out_split_stats);
int32_t mi_engine_rf_distances_device(mi_engine* engine, void* stream, int32_t tree_count, int32_t taxon_count,
                                      const int32_t* split_index, const double* branch_lengths,
                                      int32_t* out_rf, double* out_branch_score);
int32_t mi_engine_reserve_splits(mi_engine* engine, int32_t tree_count, int32_t taxon_count);
/* The device forms of the SBN calls: every array a device pointer.  index, log_prob and normalize
 * only enqueue; errors of the inputs go to the status word (mi_engine_check_status).  After
 * mi_engine_reserve_sbn(engine, tree_count, taxon_count), log_prob and normalize calls of at most
 * that many trees of that taxon count, with at most 7 tree_count (2n-3) parameters, allocate
 * nothing and synchronise nothing: they can be captured in a hipGraph.  mi_engine_sbn_train_device
 * reads one double per EM iteration and so synchronises the stream: it cannot be captured.  A
 * sharded handle reserves on its first shard. */
int32_t mi_engine_sbn_index_device(mi_engine* engine, void* stream, int32_t tree_count, int32_t taxon_count,
                                   const int32_t* parent_ids, int32_t support_tree_count,
                                   int32_t rootsplit_capacity, int32_t pcsp_capacity, int32_t* out_root_index,
                                   int32_t* out_slot_index, int32_t* out_counts, uint32_t* out_split_bits,
                                   int32_t* out_pcsp_clades, int32_t* out_parent_range, int32_t* out_pcsp_parent);
int32_t mi_engine_sbn_log_prob_device(mi_engine* engine, void* stream, int32_t tree_count, int32_t taxon_count,
                                      const int32_t* parent_ids, const int32_t* root_index,
                                      const int32_t* slot_index, int32_t rootsplit_count, int32_t pcsp_count,
                                      int32_t parent_count, const int32_t* parent_range, const double* log_params,
                                      int32_t normalized, const double* tree_weights, double* out_rooting_log_prob,
                                      double* out_log_q, double* out_log_expected_counts);
int32_t mi_engine_sbn_normalize_device(mi_engine* engine, void* stream, int32_t rootsplit_count, int32_t pcsp_count,
                                       int32_t parent_count, const int32_t* parent_range, const double* log_params,
                                       double* out_log_params);
int32_t mi_engine_sbn_train_device(mi_engine* engine, void* stream, int32_t tree_count, int32_t taxon_count,
                                   const int32_t* parent_ids, const int32_t* root_index, const int32_t* slot_index,
                                   int32_t rootsplit_count, int32_t pcsp_count, int32_t parent_count,
                                   const int32_t* parent_range, const double* tree_weights, int32_t method,
                                   double alpha, int32_t max_iter, double score_epsilon, double* out_log_params,
                                   double* out_score_history, int32_t* out_iterations);
int32_t mi_engine_reserve_sbn(mi_engine* engine, int32_t tree_count, int32_t taxon_count);
/* The device forms of the descent table, the sampler and the topology gradient: they only enqueue
 * and report through the status word; after mi_engine_reserve_sbn as above they allocate nothing
 * and read nothing back, so all three can be captured. */
int32_t mi_engine_sbn_descent_device(mi_engine* engine, void* stream, int32_t support_tree_count,
                                     int32_t taxon_count, const int32_t* parent_ids, const int32_t* root_index,
                                     const int32_t* slot_index, int32_t rootsplit_count, int32_t pcsp_count,
                                     const int32_t* pcsp_parent, int32_t* out_descent);
int32_t mi_engine_sbn_sample_device(mi_engine* engine, void* stream, int32_t sample_count, int32_t taxon_count,
                                    int32_t rootsplit_count, int32_t pcsp_count, int32_t parent_count,
                                    const int32_t* parent_range, const int32_t* descent, const double* log_params,
                                    uint64_t seed, int64_t first_sample, int32_t* out_parent_ids,
                                    int32_t* out_root_edge, int32_t* out_sampled_params, double* out_log_prob,
                                    double* out_cdf);
int32_t mi_engine_sbn_topology_gradient_device(mi_engine* engine, void* stream, int32_t tree_count,
                                               int32_t taxon_count, const int32_t* parent_ids,
                                               const int32_t* root_index, const int32_t* slot_index,
                                               int32_t rootsplit_count, int32_t pcsp_count, int32_t parent_count,
                                               const int32_t* parent_range, const double* log_params,
                                               int32_t normalized, const double* log_f, int32_t estimator,
                                               double* out_gradient, double* out_factors, double* out_log_q);
/* The device forms of PSP indexing and the branch-length models: every pointer a
 * device pointer; they only enqueue and report through the status word.  The table, the index and
 * the sample call need no workspace; after mi_engine_reserve_branch_model(engine, tree_count,
 * taxon_count, rows) the gradient call of at most that many trees and rows of that taxon count
 * allocates nothing either (its keys, its sort's workspace, the status word), and none of them
 * reads anything back: a whole step can be captured in a hipGraph.  A sharded handle reserves on
 * its first shard. */
int32_t mi_engine_psp_table_device(mi_engine* engine, void* stream, int32_t rootsplit_count, int32_t pcsp_count,
                                   const int32_t* pcsp_clades, int32_t* out_psp_of_pcsp, int32_t* out_counts);
int32_t mi_engine_psp_index_device(mi_engine* engine, void* stream, int32_t tree_count, int32_t taxon_count,
                                   const int32_t* root_index, const int32_t* slot_index, int32_t rootsplit_count,
                                   int32_t pcsp_count, const int32_t* psp_of_pcsp, int32_t variable_count,
                                   int32_t rows, int32_t* out_index);
int32_t mi_engine_branch_model_sample_device(mi_engine* engine, void* stream, int32_t tree_count,
                                             int32_t taxon_count, int32_t rows, const int32_t* index,
                                             int32_t variable_count, const double* q_params, uint64_t seed,
                                             int64_t first_sample, double prior_rate, const double* epsilon_in,
                                             double* out_branch_lengths, double* out_epsilon, double* out_log_q,
                                             double* out_log_prior);
int32_t mi_engine_branch_model_gradient_device(mi_engine* engine, void* stream, int32_t tree_count,
                                               int32_t taxon_count, int32_t rows, const int32_t* index,
                                               int32_t variable_count, const double* q_params,
                                               const double* branch_lengths, const double* epsilon,
                                               const double* log_q_branch, const double* log_prior,
                                               const double* branch_gradient, const double* log_likelihoods,
                                               const double* log_q_topology, const double* tree_weights,
                                               double beta, double prior_rate, double* out_gradient,
                                               double* out_log_f);
int32_t mi_engine_reserve_branch_model(mi_engine* engine, int32_t tree_count, int32_t taxon_count, int32_t rows);

/* ---- a device-resident variational fit (an extension) ----
 * What the reference's Burrito.gradient_steps does with vip/optimizers.py (SimpleOptimizer) and
 * vip/sgd_server.py (adam): the state of a fit lives in device memory, one step is one chain of
 * launches that reads and advances it, the optimiser is a kernel and a whole fit is one call.
 *
 * The state: the two tables (log_params [P] of the SBN, unnormalised; q_params [V][2]), Adam's
 * first and second moments of both, and the scalars
 *   t   steps so far, failed ones included      a   successful steps
 *   b0 = adam_beta0^a, b1 = adam_beta1^a: one rounded multiply per successful step, from 1
 *   step_size[2] (the mu and the sigma column of q_params), sbn_step_size, first_sample
 * Step t draws the samples s = first_sample + t K + k, k = 0 .. K-1, with the Philox layout of
 * mi_engine_sbn_sample and mi_engine_branch_model_sample under `seed`: its particles are bit for
 * bit what those calls give for (seed, first_sample + t K).  Its beta is 1 if anneal_steps is 0,
 * else max(min((t + 1) / anneal_steps, 1), 0.001) with one rounded division (burrito.py:119-121).
 *
 * One step (mi_vi_step_device) enqueues on one stream: sbn_sample, sbn_index (the support trees
 * and the samples behind them), psp_index, branch_model_sample, the unrooted gradient call,
 * sbn_log_prob, branch_model_gradient (which scales log L by beta in log_f), sbn_topology_gradient
 * with the fit's estimator, and the update below.  It allocates nothing, synchronises nothing and
 * reads nothing back: a caller may capture it in a hipGraph, and every replay is the NEXT step.
 *
 * The update (mi_vi_update*; elements are the P SBN parameters with step sbn_step_size, then
 * q_params with its column's step).  The step FAILS if any entry of either gradient is not finite
 * (the reference checks the q gradient only) or if the sigma of any split variable j < S would be
 * <= 0 or not finite after it (the reference lets that through).  Every edge's sigma is one split
 * variable's plus, with rows = 3, two PSP variables' corrections, which start at zero
 * (lognormal_mode_match) and may take either sign: they are not checked, and an edge whose SUM
 * leaves the positive numbers is reported by the next step's draw (kBranchModelBadParam).  A fit
 * of the tables alone (below) checks every variable.  A failed step changes no table and no moment and halves
 * step_size[0] and step_size[1].  Otherwise b0 and b1 are advanced first and, per element, every
 * operation rounded once in the order of the parentheses (sgd_server.py:51-67, decay 0, ascent):
 *   m = (beta0 m) + ((1 - beta0) g)
 *   v = (beta1 v) + ((1 - beta1) (g g))
 *   param = param + ((step (m / (1 - b0))) / (root + epsilon)),  root = sqrt(v / (1 - b1))
 * Where |g| > 2^500 the square g g may overflow: v is then +inf and is stored so (as the reference's
 * grad ** 2 gives it; that element's later steps are zero), while this step's root is taken of the
 * same sum in a scaled range, c = 2^-600:  v' = (beta1 ((v c) c)) + ((1 - beta1) ((g c) (g c))),
 * root = sqrt(v' / (1 - b1)) / c.  The products with c are exact (but for the underflow of
 * (v c) c, a term then 2^800 times smaller than the other), so this root is the plain one wherever
 * the plain one is finite, and a first step from zero moments is step g / (|g| + epsilon) at any g.
 * then step_size[.] *= step_decay (sbn_step_size stays, as in the reference).  Either way t += 1.
 * The step writes trace row [t] of [max_steps][6] (nothing beyond the capacity):
 *   0 beta of the step
 *   1 elbo   (sum_k f_k) / K, f_k = ((logL_k + log prior_k) - log q_topology_k) - log q_branch_k
 *            (at beta = 1 whatever the annealing), added in ascending k with one accumulator
 *   2 bound  (m + log(sum_k exp(f_k - m))) - log K, m the maximum, the sum in ascending k
 *            (the reference's marginal_likelihood_estimate); -inf if every f_k is
 *   3, 4     step_size[0], step_size[1] after the step      5  1 if the step succeeded, else 0
 *
 * mi_vi_default_options fills the reference's values: rows 3, estimator VIMCO, prior_rate 10,
 * sbn_step_size 0.001, step_decay 0.99, adam 0.9 / 0.999 / 1e-8, particle_count 10, max_steps
 * 1000, step_size {0.001, 0.001}, the rest 0.  mi_engine_vi_create takes the struct as it is. */
typedef struct mi_vi mi_vi;
typedef struct {
  int32_t particle_count;  /* K >= 1 (VIMCO: >= 2) */
  int32_t rows;            /* 1 (the split model) or 3 (the PSP model) */
  int32_t estimator;       /* MI_SBN_FACTORS_PLAIN or MI_SBN_FACTORS_VIMCO */
  int32_t anneal_steps;    /* >= 0 */
  int32_t max_steps;       /* >= 1: rows of the trace buffer */
  int32_t reserved0;
  double prior_rate;       /* finite, > 0 */
  double step_size[2];     /* finite, > 0 */
  double sbn_step_size;    /* finite, >= 0 */
  double step_decay;       /* in (0, 1] */
  double adam_beta0, adam_beta1; /* in [0, 1) */
  double adam_epsilon;     /* finite, >= 0 */
  uint64_t seed;
  int64_t first_sample;
  int32_t reserved[4];
} mi_vi_options;
int32_t mi_vi_default_options(mi_vi_options* out_options);
/* A fit on a single-device engine of 4 or 20 states (a handle of several shards is refused, one
 * of a single shard serves as its one engine: the fit's calls then report there).  The support
 * is that of parent_ids [support_tree_count][2n-3]; creation runs mi_engine_sbn_index,
 * mi_engine_sbn_descent and mi_engine_psp_table on it once, reserves what a step needs
 * (mi_engine_reserve_sbn for support_tree_count + K trees, mi_engine_reserve for K gradient
 * evaluations, mi_engine_reserve_branch_model) and allocates every buffer of a step.
 * parameter_count and variable_count must be the support's P and V (rows = 1: V = S).
 * model_params [param_count] or NULL: the one model parameter row every particle takes.
 * support_tree_count 0 (parent_ids NULL) makes a fit of the two tables alone, of any sizes
 * parameter_count + 2 variable_count >= 1: it takes mi_vi_update*, the state calls and nothing else.
 * mi_vi_destroy releases everything the fit holds (mi_device_bytes_held); the engine must outlive
 * the fit. */
int32_t mi_engine_vi_create(mi_engine* engine, int32_t support_tree_count, const int32_t* parent_ids,
                            const double* model_params, int32_t parameter_count, const double* log_params,
                            int32_t variable_count, const double* q_params, const mi_vi_options* options,
                            mi_vi** out_fit);
void mi_vi_destroy(mi_vi* fit);
/* out_sizes [9]: n, K, rows, S, C, parent_count, V, max_steps, P */
int32_t mi_vi_sizes(const mi_vi* fit, int32_t* out_sizes);
/* Enqueue one step on `stream` (NULL: the engine's).  Errors of the inputs go to the engine's
 * status word (mi_engine_check_status). */
int32_t mi_vi_step_device(mi_vi* fit, void* stream);
/* `steps` steps on the engine's stream with mi_engine_check_status after every check_interval
 * of them (<= 0: only at the end), then the trace rows of these steps into out_trace [steps][6].
 * Refused if the fit's t + steps exceeds max_steps.  The bits of a fit depend on the options, the
 * initial state, the support and the alignment alone: not on check_interval, not on how the steps
 * are split over calls, not on whether steps were replayed from a graph.
 * mi_engine_last_call_path: "vi_fit n=<n> K=<K> rows=<R> steps=<s> | <the gradient call's path>". */
int32_t mi_vi_fit(mi_vi* fit, int32_t steps, int32_t check_interval, double* out_trace);
/* Trace rows [first_step, first_step + count) into out_trace [count][6]; they must lie below both
 * the fit's t and max_steps (the rows of steps a caller's graph replayed are read this way).
 * Synchronises the engine's stream. */
int32_t mi_vi_trace(mi_vi* fit, int32_t first_step, int32_t count, double* out_trace);
/* One update of the fit's state from given gradients and per-particle terms (what the last three
 * launches of a step do): sbn_gradient [P], q_gradient [V][2], and log_likelihoods, log_prior,
 * log_q_topology, log_q_branch [K] each.  out_trace_row [6] or NULL.  The device form only
 * enqueues; every pointer a device pointer. */
int32_t mi_vi_update(mi_vi* fit, const double* sbn_gradient, const double* q_gradient, const double* log_likelihoods,
                     const double* log_prior, const double* log_q_topology, const double* log_q_branch,
                     double* out_trace_row);
int32_t mi_vi_update_device(mi_vi* fit, void* stream, const double* sbn_gradient, const double* q_gradient,
                            const double* log_likelihoods, const double* log_prior, const double* log_q_topology,
                            const double* log_q_branch, double* out_trace_row);
/* The whole state, for a checkpoint: a fit resumed from it goes on bit for bit.
 *   log_params [P], q_params [V][2], sbn_moments [2][P] (m, then v), q_moments [2][V][2]
 *   scalars [5]: b0, b1, step_size[0], step_size[1], sbn_step_size
 *   counters [3]: t, a, first_sample
 * Both synchronise the engine's stream. */
int32_t mi_vi_get_state(mi_vi* fit, double* out_log_params, double* out_q_params, double* out_sbn_moments,
                        double* out_q_moments, double* out_scalars, int64_t* out_counters);
int32_t mi_vi_set_state(mi_vi* fit, const double* log_params, const double* q_params, const double* sbn_moments,
                        const double* q_moments, const double* scalars, const int64_t* counters);
/* The last step's particles: out_parent_ids [K][2n-3] is required, the others may be NULL:
 * out_branch_lengths [K][2n-2], and out_log_likelihoods, out_log_q_topology, out_log_q_branch,
 * out_log_prior [K] each.  Synchronises the engine's stream.  A fit over a subsplit DAG
 * (mi_gp_vi_create) has rooted particles: it is refused here and served by mi_gp_vi_particles. */
int32_t mi_vi_particles(mi_vi* fit, int32_t* out_parent_ids, double* out_branch_lengths, double* out_log_likelihoods,
                        double* out_log_q_topology, double* out_log_q_branch, double* out_log_prior);

/* ---- generalized pruning: the marginal likelihood over a subsplit DAG ----
 *
 * What the reference's GPInstance / GPEngine / SubsplitDAG do (src/gp_instance.*, gp_engine.*,
 * gp_dag.*, subsplit_dag.*): the likelihood marginalised over EVERY tree of the subsplit DAG of a
 * batch of rooted topologies, in two sweeps over the DAG; per entry (GPCSP) the marginal
 * restricted to the trees that use it; the SBN parameters that follow; branch lengths per entry;
 * and the quartet hybrid marginals (mi_gp_hybrid_marginals below).
 *
 * A mi_gp is bound to a single-device 4-state engine with ONE rate category (20 states, K > 1 and
 * a handle of several shards are refused with a message; a handle of one shard serves as its one
 * engine).  It keeps the DAG, its vectors, b[G] and q[G] in device memory, counted by
 * mi_device_bytes_held; mi_gp_destroy releases them; the engine must outlive it.
 *
 * The DAG and its numbering (the reference numbers by unordered_map iteration; this rule is the
 * project's own and is deterministic):
 *   nodes    0..n-1 the leaves; then every distinct subsplit of the batch, numbered by first
 *            occurrence scanning the trees in order and, within a tree, the nodes in id order.
 *            A subsplit has two clades: clade 0 holds its lowest taxon (the reference's "sorted"
 *            side), clade 1 is the other ("rotated").
 *   entries  0..R-1 the rootsplits in order of first occurrence (as in the reference, a rootsplit
 *            is an entry); then one contiguous block per (node, clade), blocks by node id then
 *            clade, inside a block by child node id.  The entries of a block are the union over
 *            the trees of the parent -> child pairs, leaves included, so the DAG spans every
 *            combination of its entries: more trees than were given.
 *   level    of a node: its clade size (children have smaller, parents larger levels).
 *
 * Initial values: q is SubsplitDAG::BuildUniformOnTopologicalSupportPrior; b is 0.1 on every
 * entry (GPEngine's default_branch_length_), or with branch_lengths [T][2n-1] given
 * HotStartBranchLengths: the mean over the trees that hold the entry; 0 on rootsplit entries, always.
 *
 * The vectors carry one integer exponent per pattern (true value = stored x 2^e); sums align their
 * terms to the least-scaled one and a vector whose largest entry falls below rescaling_threshold
 * is scaled by a power of two.  All of that is exact, so results do not depend on the threshold
 * beyond where underflow would otherwise set in.  rescaling_threshold 0: the default 2^-256.
 *
 * Every sum over a block's entries or the entries into a node runs in entry order; every sum over
 * patterns runs tile by tile of 64 (within a tile a fixed butterfly, then the tiles ascending).
 * No float atomics: results are bit-identical however calls are batched or replayed. */
typedef struct mi_gp mi_gp;
int32_t mi_engine_gp_create(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                            const int32_t* parent_ids /* [T][2n-2] */,
                            const double* branch_lengths /* [T][2n-1] or NULL */,
                            const double* model_params /* [param_count] or NULL */, double rescaling_threshold,
                            mi_gp** out_gp);
void mi_gp_destroy(mi_gp* gp);
/* out_sizes [8]: n, node_count, rootsplit_count R, G, P, W = words of a clade bitset, levels,
 * the kernels' pattern tile width */
int32_t mi_gp_sizes(const mi_gp* gp, int32_t* out_sizes);
/* Any pointer may be NULL.  out_entries [G][3] (parent node, clade, child node; a rootsplit entry
 * is (-1, -1, its node)); out_block_range [node_count][2][2] (begin, end; a leaf: 0, 0);
 * out_clades [node_count][2][W] (bit x of word x / 32; a leaf: its bit in clade 0);
 * out_levels [node_count]; *out_topology_count = SubsplitDAG::TopologyCount. */
int32_t mi_gp_structure(const mi_gp* gp, int32_t* out_entries, int32_t* out_block_range, uint32_t* out_clades,
                        int32_t* out_levels, double* out_topology_count);
/* The entries' names as GPInstance::PrettyIndexer gives them, separated by '\n': a rootsplit is its
 * smaller chunk's bit string (taxon 0 first), a PCSP "<sister>|<focal>|<the child's smaller chunk>"
 * (zeros for a leaf child).  *out_needed (or NULL): bytes with the final 0; buffer NULL only asks. */
int32_t mi_gp_strings(const mi_gp* gp, char* buffer, int64_t capacity, int64_t* out_needed);
/* b and q, [G] each (count must be G).  Rootsplit entries of b are stored as 0.  q is taken as
 * given: normalised per block and over the rootsplits by the caller.  All four synchronise. */
int32_t mi_gp_set_branch_lengths(mi_gp* gp, const double* branch_lengths, int32_t count);
int32_t mi_gp_get_branch_lengths(mi_gp* gp, double* out_branch_lengths);
int32_t mi_gp_set_sbn_parameters(mi_gp* gp, const double* q, int32_t count);
int32_t mi_gp_get_sbn_parameters(mi_gp* gp, double* out_q);
/* SubsplitDAG::UnconditionalNodeProbabilities [node_count] and InvertedGPCSPProbabilities [G] of a
 * normalised q given in host memory (host code). */
int32_t mi_gp_node_probabilities(const mi_gp* gp, const double* q, int32_t count, double* out);
int32_t mi_gp_inverted_probabilities(const mi_gp* gp, const double* q, int32_t count, double* out);
/* Both sweeps (GPInstance::PopulatePLVs) at the object's b and q, and with them the sums every call
 * below reads.  The device form only enqueues: one launch per level and sweep, nothing allocated
 * or synchronised, so it can be captured in a hipGraph.
 * mi_engine_last_call_path: "gp_populate n=<n> nodes=<nodes> G=<G> levels=<levels> tiles=<tiles>". */
int32_t mi_gp_populate(mi_gp* gp);
int32_t mi_gp_populate_device(mi_gp* gp, void* stream);
/* out_per_gpcsp_log_likelihood [G] (GPEngine::GetPerGPCSPLogLikelihoods): sum_p w_p log l_e, the
 * likelihood restricted to the trees through e WITHOUT the factor q_e; a rootsplit row is the value
 * conditional on the rootsplit, sum_p w_p log(pi . p(root node)).  *out_log_marginal
 * (GetLogMarginalLikelihood): sum_p w_p log M_p.  Optional: out_pattern_log_marginal [P] = log M_p
 * and out_matrix [G][P] = log l_e per pattern.  The host form populates first when b or q changed
 * since the last populate (always when the matrix is asked for); the device form reads the last
 * populate's sums and takes device pointers, either may be NULL. */
int32_t mi_gp_likelihoods(mi_gp* gp, double* out_per_gpcsp_log_likelihood, double* out_log_marginal,
                          double* out_pattern_log_marginal, double* out_matrix);
int32_t mi_gp_likelihoods_device(mi_gp* gp, void* stream, double* out_per_gpcsp_log_likelihood,
                                 double* out_log_marginal);
/* Per entry, any pointer may be NULL: out_ll_derivative [G][2] = (sum_p w_p log l_e,
 * sum_p w_p l'_e / l_e), GPEngine's LogLikelihoodAndDerivative pair; and of the MARGINAL
 *   out_gradient [G]  g_e = sum_p w_p q_e l'_e / M_p   (the exact gradient of log_marginal in b_e)
 *   out_hessian  [G]  H_e = sum_p w_p [q_e l''_e / M_p - (q_e l'_e / M_p)^2]
 *   out_gsq      [G]  S_e = sum_p w_p (q_e l'_e / M_p)^2
 * with the exponents accounted for; rootsplit rows are 0.  Host form: as above. */
int32_t mi_gp_branch_derivatives(mi_gp* gp, double* out_ll_derivative, double* out_gradient, double* out_hessian,
                                 double* out_gsq);
int32_t mi_gp_branch_derivatives_device(mi_gp* gp, void* stream, double* out_ll_derivative, double* out_gradient,
                                        double* out_hessian, double* out_gsq);
/* GPInstance::EstimateSBNParameters: populate, likelihoods, then for the rootsplits and per block
 * q <- softmax(per_gpcsp_log_likelihood + log q), one logsumexp per block with the entries in
 * order; a block of one entry gets 1.  out_q [G] or NULL. */
int32_t mi_gp_estimate_sbn_parameters(mi_gp* gp, double* out_q);
/* Quartet hybrid marginals (GPInstance::CalculateHybridMarginals, GPDAG::QuartetHybridRequestOf,
 * GPEngine::CalculateQuartetHybridLikelihoods).  A central entry e = (t,c) -> s has
 * four lists of entries:
 *   rootward  the entries g = (u,cu) -> t into t, rootsplit entries excluded, ascending
 *   sister    the entries sigma of block(t, 1-c)
 *   rotated   the entries rho of block(s, 1)
 *   sorted    the entries o of block(s, 0)
 * and is FULLY FORMED iff none is empty (t is no rootsplit node and s no leaf; a rootsplit entry is
 * never central).  One summand per (g, sigma, rho, o), numbered with g outermost and o innermost;
 * per pattern, with P transposed on the two leafward steps,
 *   A = P(b_g)^T r(u,cu)   B = P(b_sigma) p(child_sigma)   C = P(b_e)^T (A o B)
 *   D = P(b_rho) p(child_rho)   E = P(b_o) p(child_o)      l_p = sum_i C_i D_i E_i
 *   summand = log(inv[g] q_sigma q_rho q_o) + sum_p w_p (log l_p - log Pr(u))
 *   hybrid[e] = logsumexp of e's summands in that order
 * with Pr = UnconditionalNodeProbabilities and inv = InvertedGPCSPProbabilities of the object's q,
 * computed on the device.  An entry that is not fully formed gets -inf; a summand whose l_p is 0 at
 * a pattern of positive weight is -inf and drops out of the logsumexp (all of them: -inf, never
 * NaN).  The vectors' exponents are accounted for, so, unlike the reference, rescaled DAGs are
 * served.  Sums over patterns run tile by tile as everywhere in mi_gp; no float atomics.
 *
 * mi_gp_hybrid_requests (host tables, any pointer may be NULL): out_requests [G][3] = (formed,
 * first summand, summand count) per entry; out_summand_entries [S][4] = the entries (g, sigma, rho,
 * o) of every summand in summand order (written on demand from the lists: the object keeps nothing
 * of size S before mi_gp_reserve_hybrid); *out_summand_count = S.
 * mi_gp_reserve_hybrid allocates what the kernels need beyond the object's vectors: per entry the
 * evolved vectors P(b_e) p(child_e) and P(b_e)^T r(t,c), the partial sums [S][tiles] and the
 * summands [S]; counted by mi_device_bytes_held, refused when over MI_PHYLO_PLV_BYTES.
 * Limits.  S grows with the product of four list lengths.  A DAG whose requests have more than
 * 2^28 summands in all is still created and serves every other call, at no cost that grows with
 * S, but mi_gp_hybrid_requests, mi_gp_reserve_hybrid, both forms of mi_gp_hybrid_marginals and
 * mi_gp_estimate_sbn_parameters_hybrid refuse it with a message; so does mi_gp_reserve_hybrid a
 * DAG of more than 65535 entries (the kernels take an entry per workgroup row).
 * mi_gp_hybrid_request_count is host code that needs no engine and no device: the number of fully
 * formed requests and S of the DAG that mi_engine_gp_create would build from the batch, refused
 * with the same message when S exceeds max_summands (0: 2^28; at most 2^28).
 * Concurrency.  A hybrid call recomputes Pr and inv from the q on the device each time (q may have
 * been written there since, and the device form may not look) and, like populate, writes scratch
 * that belongs to the object: calls of ONE object must not run concurrently on different streams.
 * mi_gp_hybrid_marginals_device only enqueues (device pointers out_hybrid [G], out_summands [S] or
 * NULL); it reads the vectors and matrices of the LAST populate and is refused before
 * mi_gp_reserve_hybrid.  mi_gp_hybrid_marginals is the host form: it reserves on first use,
 * populates first when b or q changed since (after mi_gp_optimize_branch_lengths too), synchronises.
 * mi_engine_last_call_path: "gp_hybrid formed=<formed entries> summands=<S> tiles=<tiles> z=<z>"
 * (z: over how many workgroups the summand kernel deals a request's (rootward, sister) pairs;
 * MI_PHYLO_GP_HYBRID_Z; no result depends on it). */
int32_t mi_gp_hybrid_requests(const mi_gp* gp, int32_t* out_requests, int32_t* out_summand_entries,
                              int32_t* out_summand_count);
int32_t mi_gp_hybrid_request_count(int32_t tree_count, int32_t taxon_count, const int32_t* parent_ids /* [T][2n-2] */,
                                   int64_t max_summands, int32_t* out_formed, int64_t* out_summand_count);
int32_t mi_gp_reserve_hybrid(mi_gp* gp);
int32_t mi_gp_hybrid_marginals(mi_gp* gp, double* out_hybrid, double* out_summands);
int32_t mi_gp_hybrid_marginals_device(mi_gp* gp, void* stream, double* out_hybrid, double* out_summands);
/* mi_gp_estimate_sbn_parameters with the reference's rule for hybrid marginals
 * (UpdateSBNProbabilities): a block whose entries ALL have a finite hybrid marginal takes
 * q <- softmax(hybrid + log q); any other block, and the rootsplits always, the per-entry form. */
int32_t mi_gp_estimate_sbn_parameters_hybrid(mi_gp* gp, double* out_q);
/* Maximise log_marginal over all of b at once with the rule of
 * mi_engine_optimize_branch_lengths_unrooted (accept / halve alpha, Newton step on c = -H or S,
 * step limits, projected-gradient criterion): the DAG takes the part of one tree of G - R branches,
 * an evaluation is one populate at the trial point.  Rootsplit entries stay 0.  options NULL: that
 * call's defaults with min_length e^-13.9 and max_length e^1.1 (the reference's bounds);
 * pack_active is ignored.  out_trace [max_iterations] or NULL: the accepted log_marginal after each
 * evaluation (*out_evaluations of them); *out_status: MI_BRANCH_OPT_CONVERGED, _ITERATION_LIMIT or
 * _STALLED.  This is not the reference's sequential Brent sweep over one entry at a time. */
int32_t mi_gp_optimize_branch_lengths(mi_gp* gp, const mi_branch_opt_options* options, double* out_trace,
                                      int32_t* out_evaluations, int32_t* out_status);

/* ---- trees of the subsplit DAG: index, log q, training, sampling, enumeration ----
 *
 * With its q a mi_gp is a ROOTED subsplit Bayesian network (the reference's RootedSBNInstance and
 * the tree side of GPInstance: TrainSimpleAverage, GenerateCompleteRootedTreeCollection,
 * CurrentlyLoadedTreesWithGPBranchLengths).  A rooted tree is in the form mi_engine_gp_create
 * takes: parent_ids [2n-2], leaves 0..n-1, every parent id above its children's, the root 2n-2,
 * with the same checks; a refused tree is named in the engine's status word (a host form returns
 * the error; mi_engine_check_status reports it after a device form), its entries are G and its
 * nodes -1.  A tree the library BUILDS (sampled or enumerated) is numbered by one rule -- leaves
 * 0..n-1 by taxon, internal nodes in post-order, children ordered by largest leaf id, the root
 * 2n-2 --, under which a topology has exactly one id vector.
 *
 * mi_engine_gp_create_dag makes a DAG-ONLY object on ANY engine (4 or 20 states, any number of
 * rate categories; a handle of several shards serves with its first shard): the same DAG,
 * numbering, initial q and b as mi_engine_gp_create, and no model, tip codes or vectors.  The
 * structure, string, b / q, probability and hybrid-request table calls and every call of this
 * section serve it; populate, likelihoods, branch_derivatives, estimate_sbn_parameters, the hybrid
 * marginals and optimize_branch_lengths refuse it with a message that says so.
 *
 * mi_gp_reserve_trees uploads what the tree calls read -- the clade words, a table from subsplit
 * to node (open addressing, keyed by a hash of the two clades' W words; a candidate is CONFIRMED by
 * comparing the clade words, so identification is exact), the rootsplit entry of every node and,
 * as uint64 saturated at 2^62, the number of topologies below every node -- and allocates the
 * workspace for tree_capacity trees, counted by mi_device_bytes_held and refused with
 * the sizes in the message when over MI_PHYLO_PLV_BYTES (a batch is not chunked).  After it the
 * *_device forms of at most tree_capacity trees allocate nothing, synchronise nothing and can be
 * captured in a hipGraph; before it, or with more trees, they are refused.  Reserving MORE
 * reallocates: re-capture.  The host forms reserve on first use.  Calls of one object must not
 * run concurrently on different streams.  Device forms take device pointers.
 *
 * mi_gp_tree_index: out_nodes [T][2n-1] (or NULL) the DAG node of every tree node (a leaf: its
 * taxon; a subsplit the DAG does not hold: -1); out_entries [T][2n-1]: for v < 2n-2 the entry
 * (node(parent v), clade, node(v)), found by bisection of the block (parent, clade), which is
 * sorted by child node; for v = 2n-2 the rootsplit entry of the root's node.  Whatever is not in
 * the DAG is the sentinel G: an unknown node at either end, a pair missing from its block, a root
 * that is no rootsplit.
 * mi_engine_last_call_path: "gp_trees n=<n> T=<T> store=lds|global" (a lane per tree; the tree's
 * node words are in LDS while at least 8 trees' fit into 64 KiB, else in the workspace;
 * MI_PHYLO_GP_TREES_STORE=global, read when the engine is created, keeps them in the workspace at
 * every size: same bits).
 *
 * mi_gp_tree_log_prob: out_log_q[t] = sum over v = 0 .. 2n-2 ascending, one accumulator, of
 * log q[entries[t][v]] at the object's q (taken as given).  A sentinel (anything outside [0, G))
 * or a zero parameter gives -inf, never NaN.
 * mi_gp_tree_branch_lengths (TreesWithGPBranchLengthsOfTopologies): b[entries[t][v]] per node,
 * missing_length at a sentinel, 0 at the root.
 *
 * mi_gp_train_simple_average (the rooted TrainSimpleAverage; host pointers): per entry the sum of
 * the weights (NULL: 1 each; finite, not negative) of the trees that use it, in ascending tree
 * order (a stable sort by entry; the head of a run adds its run); then q = count / (the sum over
 * the rootsplits, or over the entry's block, in entry order); a block whose total is 0 gets zeros.
 * A tree with a sentinel is an error that names the tree, and q stays as it was.  The result is
 * set as the object's q and copied to out_q [G] (or NULL).
 *
 * mi_gp_sample_trees: K rooted trees drawn from q.  cdf[j] = sum_{i <= j} q_i per block and over
 * the rootsplits, ascending, one accumulator (out_cdf [G] or NULL); a negative, NaN or infinite q
 * is refused.  Philox4x32-10 keyed and countered exactly as mi_engine_sbn_sample states: draw i of
 * sample t = first_sample + k has key seed and counter (i, 0, t lo, t hi), u = (the first two
 * output words as one 64-bit number >> 11) 2^-53, and picks the smallest j with
 * cdf[j] > u cdf[e-1] (if there is none, the smallest j with cdf[j] == cdf[e-1]).  Draw 0 picks
 * the rootsplit; at a node clade 0's block is drawn, then that child's subtree is descended depth
 * first, then clade 1's block; every visited block takes one draw, blocks of one entry included.
 * A visited block with total 0 is an error that names the sample (its position k in the call, as
 * mi_engine_sbn_sample does, not first_sample + k) and the block; that sample's integer outputs
 * are -1, its log q and lengths NaN.  out_parent_ids [K][2n-2] by the numbering
 * rule; out_entries [K][2n-1] and out_log_q [K] are bit for bit what mi_gp_tree_index and
 * mi_gp_tree_log_prob give for the tree; out_branch_lengths [K][2n-1] (or NULL) what
 * mi_gp_tree_branch_lengths gives.  A sample's bits depend on (seed, t) alone.
 *
 * mi_gp_enumerate_trees: trees first .. first + count - 1 of the DAG by unranking in uint64 (the
 * order of tests/gp_ref.py: enumerate_trees): the rootsplits in entry order by the running sum of
 * the counts below them; at a node clade 0 is the slow digit and clade 1 the fast one; inside a
 * clade the entries in order by the running sum of the counts below their children, the remainder
 * passing down to the child.  Same outputs as the sampler (one tree-building kernel body, two ways
 * to pick an entry).  Refused, before anything is reserved: first + count beyond the topology
 * count, or a DAG of 2^62 topologies or more.  Sampling serves a DAG of any size.
 * mi_gp_topology_count: *out_count = SubsplitDAG::TopologyCount as an integer, saturated at 2^62
 * (mi_gp_structure gives it as a double).  Host arithmetic on the DAG, done once per object; it
 * reserves and uploads nothing.
 *
 * mi_engine_deroot_trees (any engine, any n >= 3): Node::Deroot as mi_engine_sbn_sample words it.
 * The trifurcation goes to the root child that holds taxon n-1 unless that child is a leaf, then to
 * the other one; the remaining root child y becomes its third child; ids are renumbered in the
 * unrooted convention (leaves, post-order, children by largest leaf id, root 2n-3).
 * out_parent_ids [T][2n-3]; out_root_edge [T] the new id of y; with branch_lengths [T][2n-1],
 * out_branch_lengths [T][2n-2] (or NULL): every edge's length under its new id, the two root
 * edges' lengths added onto out_root_edge, 0 in the root's slot.  mi_engine_reserve_deroot
 * allocates the device form's workspace. */
int32_t mi_engine_gp_create_dag(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                                const int32_t* parent_ids /* [T][2n-2] */,
                                const double* branch_lengths /* [T][2n-1] or NULL */, mi_gp** out_gp);
int32_t mi_gp_reserve_trees(mi_gp* gp, int32_t tree_capacity);
int32_t mi_gp_topology_count(mi_gp* gp, uint64_t* out_count);
int32_t mi_gp_tree_index(mi_gp* gp, int32_t tree_count, const int32_t* parent_ids, int32_t* out_entries,
                         int32_t* out_nodes);
int32_t mi_gp_tree_index_device(mi_gp* gp, void* stream, int32_t tree_count, const int32_t* parent_ids,
                                int32_t* out_entries, int32_t* out_nodes);
int32_t mi_gp_tree_log_prob(mi_gp* gp, int32_t tree_count, const int32_t* entries, double* out_log_q);
int32_t mi_gp_tree_log_prob_device(mi_gp* gp, void* stream, int32_t tree_count, const int32_t* entries,
                                   double* out_log_q);
int32_t mi_gp_tree_branch_lengths(mi_gp* gp, int32_t tree_count, const int32_t* entries, double missing_length,
                                  double* out_branch_lengths);
int32_t mi_gp_tree_branch_lengths_device(mi_gp* gp, void* stream, int32_t tree_count, const int32_t* entries,
                                         double missing_length, double* out_branch_lengths);
int32_t mi_gp_train_simple_average(mi_gp* gp, int32_t tree_count, const int32_t* entries,
                                   const double* tree_weights /* [T] or NULL */, double* out_q);
int32_t mi_gp_sample_trees(mi_gp* gp, int32_t sample_count, uint64_t seed, int64_t first_sample,
                           int32_t* out_parent_ids, int32_t* out_entries, double* out_log_q,
                           double* out_branch_lengths, double* out_cdf);
int32_t mi_gp_sample_trees_device(mi_gp* gp, void* stream, int32_t sample_count, uint64_t seed, int64_t first_sample,
                                  int32_t* out_parent_ids, int32_t* out_entries, double* out_log_q,
                                  double* out_branch_lengths, double* out_cdf);
int32_t mi_gp_enumerate_trees(mi_gp* gp, int64_t first, int32_t count, int32_t* out_parent_ids, int32_t* out_entries,
                              double* out_log_q, double* out_branch_lengths);
int32_t mi_gp_enumerate_trees_device(mi_gp* gp, void* stream, int64_t first, int32_t count, int32_t* out_parent_ids,
                                     int32_t* out_entries, double* out_log_q, double* out_branch_lengths);
int32_t mi_engine_reserve_deroot(mi_engine* engine, int32_t tree_count, int32_t taxon_count);
int32_t mi_engine_deroot_trees(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                               const int32_t* parent_ids /* [T][2n-2] */,
                               const double* branch_lengths /* [T][2n-1] or NULL */,
                               int32_t* out_parent_ids /* [T][2n-3] */,
                               double* out_branch_lengths /* [T][2n-2] or NULL */, int32_t* out_root_edge /* [T] */);
int32_t mi_engine_deroot_trees_device(mi_engine* engine, void* stream, int32_t tree_count, int32_t taxon_count,
                                      const int32_t* parent_ids, const double* branch_lengths,
                                      int32_t* out_parent_ids, double* out_branch_lengths, int32_t* out_root_edge);

/* ---- a variational fit over the rooted trees of the subsplit DAG (an extension) ----
 *
 * The rooted counterpart of mi_engine_vi_create: the variational family is the rooted SBN of a mi_gp
 * (full or DAG-only, so any engine serves: 4 or 20 states, any number of rate categories) with one
 * log-normal branch-length variable per entry, which is what generalized pruning keeps (b[G]).
 * Notation: G entries, R rootsplits, N = 2n-1 nodes of a rooted tree (the root N-1), and blocks as
 * mi_gp_structure gives them: the rootsplits [0, R), then one block per (node, clade).  The tables
 * are log_params [G] (phi, unnormalised) and q_params [G][2] (mu, sigma of entry e); the object's
 * own q and b are read by nothing here and changed by nothing here.
 *
 * mi_gp_log_normalize: per block with maximum m,
 *   out_log_q[e] = (phi_e - m) - log(sum_{i in block} exp(phi_i - m)),  out_q[e] = exp(out_log_q[e])
 * the sum in ascending entry order with one accumulator (a lane per block).  -inf is allowed (q = 0;
 * a block that is all -inf gets log q = -inf and q = 0 throughout); NaN and +inf are an error that
 * names the entry.  out_log_q may be NULL.
 *
 * The topology side of a step is mi_gp_sample_trees with that q in the object's place: the same
 * Philox layout, entries, and log q = sum over v = 0 .. 2n-2 ascending of log q[entries[v]].
 *
 * mi_gp_branch_sample: branch lengths of tree_count rooted trees given by their entries [T][N].  Per
 * tree t and node v = 0 .. 2n-3 the variable is e = entries[t][v]; the root's slot N-1 carries its
 * rootsplit entry and no length.  A sentinel (anything outside [0, G)) is an error that names the
 * tree and the node; so is sigma_e <= 0 or not finite, or a NaN mu_e.
 *   eps = epsilon_in[t][v] if given, else the standard normal of mi_engine_branch_model_sample:
 *   Philox key (seed lo, seed hi), counter (v, 1, s lo, s hi), s = first_sample + t, the same
 *   Box-Muller form.  x = mu_e + sigma_e eps (a rounded product, a rounded sum), theta = exp(x).
 *   out_branch_lengths [T][N]  theta; 0 in the root's slot: the layout mi_engine_deroot_trees takes
 *   out_epsilon [T][N-1]
 *   out_log_q [T]      -sum_v (((x + log sigma) + log(2 pi)/2) + 0.5 (eps eps)), ascending v < N-1,
 *                      one accumulator from 0
 *   out_log_prior [T]  (2n-2) log(prior_rate) - prior_rate sum_v theta, the sum in the same order:
 *                      Exp(prior_rate) on every rooted edge
 * Rows of rootsplit entries (j < R) are carried in q_params and never drawn from.
 *
 * mi_engine_deroot_trees_mapped: mi_engine_deroot_trees with one more output,
 *   out_new_id [T][N]  the unrooted id under which every rooted node's edge lands: both root
 *                      children map to out_root_edge, the root to -1 (a refused tree: all -1)
 * so that out_branch_lengths[u] = sum over v with new_id[v] == u of branch_lengths[v], and the
 * derivative of log L with respect to a rooted edge v is the unrooted gradient's entry new_id[v]
 * (the two root edges share the merged edge's).
 *
 * mi_gp_branch_gradient: the reparametrisation gradient with respect to q_params and log_f.
 * branch_lengths, epsilon, log_q_branch, log_prior: the sample call's outputs; new_id: the mapped
 * de-rooting's; branch_gradient [T][N] and log_likelihoods [T]: mi_engine_gradients_unrooted's for
 * the de-rooted trees (2n-1 = N entries per tree).  Per (t, v), v < N-1, with g =
 * branch_gradient[t][new_id[t][v]], d = g - prior_rate, w = tree_weights[t] (1 if NULL):
 *   c0 = w ((d theta) + 1)      c1 = w ((((d theta) eps) + eps) + (1 / sigma))
 * every operation rounded once, in the order the parentheses give.
 *   out_gradient [G][2]  row j: the sum of c0 resp. c1 over the positions (t, v), v < N-1, with
 *       entries[t][v] == j, in ascending position t N + v, one accumulator per component from 0
 *       (a run of more than 16 positions is a wave's: 64 side by side, added lane after lane: the same
 *       additions in the same order).  An entry no position names, and every rootsplit row, gets 0.
 *   out_log_f [T]  ((beta log_likelihoods[t] + log_prior[t]) - log_q_topology[t]) - log_q_branch[t]
 *       (log_q_topology NULL: 0)
 *
 * mi_gp_topology_gradient: the gradient of the multi-sample objective with respect to log_params.
 * The usage of a parameter by a tree is an indicator, so
 *   G_j = sum over the trees t that use j (the root's slot included) of a_t, in ascending t with one
 *         accumulator (the same runs of the same stable sort by entry as above)
 *   out_gradient[j] = G_j - q_j sum_{i in block(j)} G_i, the block's sum in ascending entry order,
 *         q the normalised table of mi_gp_log_normalize
 * with the factors a_t from log_f by the formulas of mi_engine_sbn_topology_gradient
 * (MI_SBN_FACTORS_PLAIN, _VIMCO, _GIVEN; out_factors [T] or NULL).  Sentinel entries are skipped.
 *
 * mi_gp_reserve_vi reserves what these calls need for tree_capacity trees (it includes
 * mi_gp_reserve_trees); after it the *_device forms allocate nothing, synchronise nothing and can be
 * captured; the host forms reserve on first use.  Device forms take device pointers.
 *
 * mi_gp_vi_create: a fit whose step is the chain
 *   log-normalise, CDF and tree building (sampling), branch draw, mapped de-rooting,
 *   mi_engine_gradients_unrooted_device for K trees with the one model row, the terms, the factors,
 *   one sort and the two ordered sums, the update of mi_vi_update* with P = V = G
 * on one stream.  Step t draws the samples first_sample + t K + k and its beta from the fit's state
 * in device memory, as DESIGN.md 4.24 words it; every variable's sigma (rootsplit rows included)
 * must stay positive, else the step fails as an unrooted fit's does; a non-finite gradient entry
 * fails it too.  options->rows must be 1.  parameter_count and variable_count must both be G.
 * Creation reserves (mi_gp_reserve_trees, mi_engine_reserve for K gradient evaluations,
 * mi_engine_reserve_deroot), cuts one buffer and uploads; a step allocates nothing, synchronises
 * nothing and reads nothing back.  mi_vi_destroy releases the fit's buffer; the three reservations belong
 * to the object and the engine and stay grown, so mi_device_bytes_held is back where it was before
 * mi_gp_vi_create only when an earlier fit (or the reserve calls) had made them already.  mi_vi_step_device, mi_vi_fit, mi_vi_trace, mi_vi_update[_device],
 * mi_vi_get_state, mi_vi_set_state, mi_vi_sizes (rows 1, S = R, C = 0, V = P = G) and mi_vi_destroy
 * serve it as they serve an unrooted fit; mi_vi_particles refuses it and mi_gp_vi_particles gives
 * the last step's rooted particles: out_parent_ids [K][2n-2] (required), out_entries [K][N],
 * out_branch_lengths [K][N], and out_log_likelihoods, out_log_q_topology, out_log_q_branch,
 * out_log_prior [K] each (or NULL).  An object made on a handle of several shards is refused.  The
 * object and its engine must outlive the fit, and reserving more trees on the object invalidates a
 * captured step.  The bits of a fit depend on the options, the initial state, the DAG and the
 * alignment alone.
 * mi_engine_last_call_path: "gp_vi_fit n=<n> K=<K> G=<G> steps=<s> | <the gradient call's path>". */
int32_t mi_gp_reserve_vi(mi_gp* gp, int32_t tree_capacity);
int32_t mi_gp_log_normalize(mi_gp* gp, const double* log_params /* [G] */, double* out_log_q, double* out_q);
int32_t mi_gp_log_normalize_device(mi_gp* gp, void* stream, const double* log_params, double* out_log_q, double* out_q);
int32_t mi_gp_branch_sample(mi_gp* gp, int32_t tree_count, const int32_t* entries, const double* q_params /* [G][2] */,
                            uint64_t seed, int64_t first_sample, double prior_rate,
                            const double* epsilon_in /* [T][2n-2] or NULL */, double* out_branch_lengths,
                            double* out_epsilon, double* out_log_q, double* out_log_prior);
int32_t mi_gp_branch_sample_device(mi_gp* gp, void* stream, int32_t tree_count, const int32_t* entries,
                                   const double* q_params, uint64_t seed, int64_t first_sample, double prior_rate,
                                   const double* epsilon_in, double* out_branch_lengths, double* out_epsilon,
                                   double* out_log_q, double* out_log_prior);
int32_t mi_gp_branch_gradient(mi_gp* gp, int32_t tree_count, const int32_t* entries, const double* q_params,
                              const double* branch_lengths, const double* epsilon, const double* log_q_branch,
                              const double* log_prior, const int32_t* new_id, const double* branch_gradient,
                              const double* log_likelihoods, const double* log_q_topology /* [T] or NULL */,
                              const double* tree_weights /* [T] or NULL */, double beta, double prior_rate,
                              double* out_gradient, double* out_log_f);
int32_t mi_gp_branch_gradient_device(mi_gp* gp, void* stream, int32_t tree_count, const int32_t* entries,
                                     const double* q_params, const double* branch_lengths, const double* epsilon,
                                     const double* log_q_branch, const double* log_prior, const int32_t* new_id,
                                     const double* branch_gradient, const double* log_likelihoods,
                                     const double* log_q_topology, const double* tree_weights, double beta,
                                     double prior_rate, double* out_gradient, double* out_log_f);
int32_t mi_gp_topology_gradient(mi_gp* gp, int32_t tree_count, const int32_t* entries, const double* log_params,
                                const double* log_f, int32_t estimator, double* out_gradient, double* out_factors);
int32_t mi_gp_topology_gradient_device(mi_gp* gp, void* stream, int32_t tree_count, const int32_t* entries,
                                       const double* log_params, const double* log_f, int32_t estimator,
                                       double* out_gradient, double* out_factors);
int32_t mi_engine_deroot_trees_mapped(mi_engine* engine, int32_t tree_count, int32_t taxon_count,
                                      const int32_t* parent_ids, const double* branch_lengths,
                                      int32_t* out_parent_ids, double* out_branch_lengths, int32_t* out_root_edge,
                                      int32_t* out_new_id /* [T][2n-1] or NULL */);
int32_t mi_engine_deroot_trees_mapped_device(mi_engine* engine, void* stream, int32_t tree_count, int32_t taxon_count,
                                             const int32_t* parent_ids, const double* branch_lengths,
                                             int32_t* out_parent_ids, double* out_branch_lengths,
                                             int32_t* out_root_edge, int32_t* out_new_id);
int32_t mi_gp_vi_create(mi_gp* gp, const double* model_params, int32_t parameter_count, const double* log_params,
                        int32_t variable_count, const double* q_params, const mi_vi_options* options, mi_vi** out_fit);
int32_t mi_gp_vi_particles(mi_vi* fit, int32_t* out_parent_ids, int32_t* out_entries, double* out_branch_lengths,
                           double* out_log_likelihoods, double* out_log_q_topology, double* out_log_q_branch,
                           double* out_log_prior);

/* Synchronise `stream` and report the first per-tree error since the last check (the status
 * word is sticky and cleared when an error is reported: calls themselves never clear it). */
int32_t mi_engine_check_status(mi_engine* engine, void* stream);

/* Introspection for the bench / profiles: name and launch count of the dominant
 * kernel of the last call, and the algorithmic bytes it accounts for
 * (DESIGN.md "Measurement"). */
int32_t mi_engine_last_call_info(const mi_engine* engine, const char** dominant_kernel,
                                 int64_t* evaluations, int64_t* gradient_evaluations);
/* One line saying which path the last call took: the dominant kernel, where the partial
 * vectors were kept (store=lds | arena | hbm), whether the tree set-up rode in the walk's launch
 * (setup=in-walk) or had its own, and the call's flavour (fd=16, site-pass, light, analytic,
 * rescaled, rooted, K=...).  Diagnostics for the randomised sweeps (tools/stress_*.py print a
 * histogram of it); the string is the engine's and lives until the next call. */
const char* mi_engine_last_call_path(const mi_engine* engine);

/* How the last call was cut up: the number of launches of the walk kernel(s) over chunks of
 * evaluations (the partial-vector arena of large trees holds only as many evaluations as
 * MI_PHYLO_PLV_BYTES allows; 1 when everything went in one launch), and how many times since
 * the engine was made the arena budget had to be reduced because the device could not give
 * the memory.  Either pointer may be NULL. */
int32_t mi_engine_last_call_launches(const mi_engine* engine, int32_t* walk_launches,
                                     int32_t* arena_backoffs);

/* Kernel timing for bench.py: after mi_engine_profile_begin(engine, max_calls)
 * every call brackets its dominant kernel launch(es) with a pair of HIP events on
 * the call's stream (no synchronisation).  mi_engine_profile_collect()
 * synchronises on the recorded events, writes one duration in milliseconds per
 * profiled call and stops profiling. */
int32_t mi_engine_profile_begin(mi_engine* engine, int32_t max_calls);
int32_t mi_engine_profile_collect(mi_engine* engine, double* out_ms, int32_t capacity,
                                  int32_t* out_count);
/* The same with the call cut into four phases by five more events (a few microseconds of
 * device time per call: not for a timed region whose step time is reported):
 *   [0] set-up (tree schedules, model instances; 20 states: + the transition matrices of
 *       the first launch)          [1] post-order walk (+ root) of the FIRST walk launch (20
 *       states; 0 for the 4-state kernels, whose walks are one kernel)
 *   [2] pre-order walk of the first launch (20 states) / the main walk pass (4 states)
 *   [3] everything after it (further launches of a chunked call, finite-difference and
 *       site passes, tile reduction, finalize).
 * out_phase_ms: [capacity][4]; *out_first_launch_evaluations: evaluations the first walk
 * launch covered (what a per-launch roofline divides by). */
int32_t mi_engine_profile_begin_phases(mi_engine* engine, int32_t max_calls);
int32_t mi_engine_profile_collect_phases(mi_engine* engine, double* out_ms, double* out_phase_ms,
                                         int32_t capacity, int32_t* out_count,
                                         int32_t* out_first_launch_evaluations);

/* ---- site-pattern compression on the device (widening beyond the Engine boundary) ----
 *
 * Replaces SitePattern::Compress (src/site_pattern.cpp:77-115; called from the
 * SitePattern constructor :9-14): the distinct columns of an alignment, their
 * multiplicities, in the iteration order of the reference's
 * std::unordered_map<std::vector<int>, double, IntVectorHasher> -- bit-exact.
 *
 *   codes        [taxon_count][site_count] symbol codes 0..3, 4 = gap/ambiguous
 *                (SitePattern::SymbolVectorOf, site_pattern.cpp:16-46), rows in taxon-id
 *                order, host memory
 *   out_patterns [taxon_count][*out_pattern_count] (dense; capacity taxon_count *
 *                site_count int32), out_weights [*out_pattern_count] (capacity site_count)
 *   out_hash_kernel_ms  optional: HIP-event time of the column-hashing kernel
 * Hashing, sorting and grouping run on the GPU; the P insertions that fix the order are
 * replayed on the host.  A 64-bit grouping-hash collision (verified, never assumed absent)
 * is retried with another hash seed, so a returned result is always exact.  Fails without
 * a GPU (libmi_phylo_host.so holds the CPU implementation). */
int32_t mi_site_pattern_compress(int32_t device, int32_t taxon_count, int64_t site_count,
                                 const int8_t* codes, int32_t* out_pattern_count,
                                 int32_t* out_patterns, double* out_weights,
                                 double* out_hash_kernel_ms);
/* The device-resident form (round 4): the same compression, but the pattern matrix
 * [taxon_count][*out_pattern_count] (int32, dense) and the weights stay in device memory --
 * for a 512 x 50 000 alignment that is 82 MB that need not come down only to go up again.
 * The two arrays are allocated by the library on `device` and handed to the caller, who
 * passes them to mi_engine_create_device_tips and releases them with mi_device_free (the
 * engine keeps its own copies). */
int32_t mi_site_pattern_compress_device(int32_t device, int32_t taxon_count, int64_t site_count,
                                        const int8_t* codes, int32_t* out_pattern_count,
                                        int32_t** out_device_patterns,
                                        double** out_device_weights, double* out_hash_kernel_ms);
void mi_device_free(void* device_pointer);
/* mi_engine_create / mi_engine_create_reversible (by spec->state_count; 20 states: the
 * built-in WAG table) with the tips ALREADY ON THE DEVICE: device_tip_states[n*P] int32 (as
 * tip_states above: >= s means gap) and device_pattern_weights[P], on spec->device (the
 * current device for -1).  use_tip_states == 0 derives the 0/1 partial vectors on the device
 * as SitePattern::GetPartials does.  Results are bit-identical to an engine made from the
 * same arrays in host memory. */
int32_t mi_engine_create_device_tips(const mi_engine_spec* spec, const int32_t* device_tip_states,
                                     const double* device_pattern_weights,
                                     mi_engine** out_engine);

#ifdef __cplusplus
}
#endif
#endif /* MI_PHYLO_H_ */
