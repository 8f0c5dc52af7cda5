"""Python mirror of libsbn's Engine (src/engine.hpp:26-54) on top of the C ABI.

Names follow the reference: PhyloModelSpecification(substitution, site, clock),
Engine.log_likelihoods / gradients return what Engine::LogLikelihoods /
Engine::Gradients return (a vector of doubles / one PhyloGradient per tree with
the gradient map keys "branch_lengths", "site_model", "substitution_model",
"ratios_root_height", "clock_model").  Errors surface as RuntimeError, as
pybind11 does for the reference's Failwith (src/sugar.hpp:67-78).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi

SUBST = {"JC69": 0, "GTR": 1, "WAG": 2, "reversible": 2}
CLOCK = {"none": 0, "strict": 1}


@dataclass
class PhyloModelSpecification:
    """src/phylo_model.hpp:13-17."""
    substitution: str = "JC69"
    site: str = "constant"
    clock: str = "strict"


def wag_model():
    """The built-in WAG table as (exchangeabilities[190], frequencies[20]) -- upper triangle
    row by row, amino-acid order ARNDCQEGHILKMFPSTWYV (mi_wag_model)."""
    ex, fr = np.zeros(190), np.zeros(20)
    rc = _capi.load().mi_wag_model(ex.ctypes.data_as(_capi.F64P), fr.ctypes.data_as(_capi.F64P))
    if rc != 0:
        raise RuntimeError(_capi.last_error())
    return ex, fr


class PhyloGradient:
    """src/tree_gradient.hpp:10-19.  (A plain __slots__ class: a call returns one object
    per tree, and dataclass construction was most of the Python-side time of a call.)"""
    __slots__ = ("log_likelihood", "gradient")

    def __init__(self, log_likelihood, gradient):
        self.log_likelihood = log_likelihood
        self.gradient = gradient

    def __repr__(self):
        return f"PhyloGradient(log_likelihood={self.log_likelihood!r}, gradient={self.gradient!r})"


@dataclass
class BranchOptResult:
    """What Engine.optimize_branch_lengths returns: per tree the maximum-likelihood branch
    lengths [T][2n-2], the log-likelihood, branch gradient and Hessian diagonal [T][2n-1] at
    them, the evaluations used and the status (0 converged, 1 iteration limit, 2 stalled)."""
    branch_lengths: np.ndarray
    log_likelihood: np.ndarray
    gradient: np.ndarray
    hessian: np.ndarray
    iterations: np.ndarray
    status: np.ndarray


def _branch_opt_options(max_iterations, check_interval, pack_active, tolerance, min_length,
                        max_length):
    return _capi.BranchOptOptions(int(max_iterations), int(check_interval), int(bool(pack_active)),
                                  float(tolerance), float(min_length), float(max_length))


@dataclass
class NniSearchResult:
    """What Engine.nni_search returns: per tree the topology [T][2n-3] and branch lengths
    [T][2n-2] of its last optimisation, the log-likelihood and the largest NNI delta there, the
    moves taken, their codes 2 v + i (in the ids of the tree at that round; -1: unused) and
    deltas [T][max_moves], the status (0 local optimum, 1 move limit) and that optimisation's
    status."""
    parent_ids: np.ndarray
    branch_lengths: np.ndarray
    log_likelihood: np.ndarray
    best_delta: np.ndarray
    move_count: np.ndarray
    move_log: np.ndarray
    move_gain: np.ndarray
    status: np.ndarray
    branch_opt_status: np.ndarray


@dataclass
class SprSearchResult:
    """What Engine.spr_search returns: per tree the topology [T][2n-3] and branch lengths
    [T][2n-2] of its last optimisation, the log-likelihood and the largest SPR delta there, the
    moves taken, their triples (s, dir, f) [T][max_moves][3] (in the ids of the tree at that
    round; -1: unused) and deltas [T][max_moves], the status (0 local optimum, 1 move limit) and
    that optimisation's status."""
    parent_ids: np.ndarray
    branch_lengths: np.ndarray
    log_likelihood: np.ndarray
    best_delta: np.ndarray
    move_count: np.ndarray
    move_log: np.ndarray
    move_gain: np.ndarray
    status: np.ndarray
    branch_opt_status: np.ndarray


@dataclass
class RellResult:
    """What Engine.rell_bootstrap returns: log-likelihoods [T], per-pattern log-likelihoods
    [T][P] (unweighted), replicate log-likelihoods C [B][T], the best tree per replicate [B]
    (lowest index among equals), bootstrap proportions [T] and expected-likelihood weights [T]."""
    log_likelihood: np.ndarray
    pattern_log_likelihood: np.ndarray
    replicate_log_likelihood: np.ndarray
    best_tree: np.ndarray
    bootstrap_proportion: np.ndarray
    expected_likelihood_weight: np.ndarray


@dataclass
class TopologyTests:
    """What Engine.topology_tests and Engine.topology_tests_matrix return, per tree [T]: the
    observed log-likelihood L, L[best] - L, the bootstrap proportion and expected-likelihood
    weight of block 0, the p-values of the KH, SH and AU tests, the AU fit's d, c and residual sum
    of squares (NaN, and p_au = bp, where fewer than two scales were usable) and the usable-scale
    count; counts [K][T] (int32) the replicates each tree won per block, column_mean [T] the means
    of block 0's replicate log-likelihoods, sites and replicates [K] the blocks; `table` is the
    [T][11] matrix the columns come from.  On request replicate_log_likelihood [B_0][T] and
    best_tree [B_0] of block 0; the fused call adds tree_log_likelihood [T] (what log_likelihoods
    returns) and pattern_log_likelihood [T][P]."""
    table: np.ndarray
    log_likelihood: np.ndarray
    delta: np.ndarray
    bootstrap_proportion: np.ndarray
    expected_likelihood_weight: np.ndarray
    p_kh: np.ndarray
    p_sh: np.ndarray
    p_au: np.ndarray
    au_d: np.ndarray
    au_c: np.ndarray
    au_rss: np.ndarray
    usable_scales: np.ndarray
    counts: np.ndarray
    column_mean: np.ndarray
    sites: np.ndarray
    replicates: np.ndarray
    replicate_log_likelihood: np.ndarray = None
    best_tree: np.ndarray = None
    tree_log_likelihood: np.ndarray = None
    pattern_log_likelihood: np.ndarray = None

    @classmethod
    def from_table(cls, table, counts, mean, sites, replicates, c=None, best=None):
        cols = [np.ascontiguousarray(table[:, j]) for j in range(10)]
        return cls(table, *cols, table[:, 10].astype(np.int32), counts, mean, sites, replicates, c, best)


@dataclass
class StartingTrees:
    """What Engine.starting_trees returns: per replicate the neighbour-joining tree of its
    maximum-likelihood distances -- parent ids [B][2n-3] and branch lengths [B][2n-2] in the form
    every unrooted call takes -- and, on request, the distance matrices [B][n][n]."""
    parent_ids: np.ndarray
    branch_lengths: np.ndarray
    distances: np.ndarray = None


@dataclass
class PairwiseDistances:
    """What Engine.pairwise_distances returns: distances [B][n][n] (symmetric, zero diagonal);
    on request the substitution counts [B][n(n-1)/2][4][4] of the pairs in lexicographic (i, j)
    order and the solver's status per pair [B][n(n-1)/2] (int8: 0 converged, 1 lower bound,
    2 upper bound, 3 no data, 4 iteration limit)."""
    distances: np.ndarray
    pair_counts: np.ndarray = None
    pair_status: np.ndarray = None


def _distance_options(min_length, max_length, tolerance, max_iterations):
    return _capi.DistanceOptions(int(max_iterations), 0, float(tolerance), float(min_length),
                                 float(max_length))


@dataclass
class AncestralStates:
    """What Engine.ancestral_states returns, per tree and pattern, unweighted: the marginal
    posterior of the state at the internal nodes n .. 2n-3 [T][n-2][P][4] (row v - n: node v; the
    last row is the root) and the log-likelihoods [T]; on request the state of the largest
    posterior [T][n-2][P] (int8, the lowest among equals), the rate-category posteriors [T][P][K]
    with the posterior mean rates [T][P], and the state posteriors at the leaves [T][n][P][4]
    (the tip vector itself for an unambiguous tip, an imputation otherwise).  A pattern of
    likelihood 0 has NaN rows and map state 0."""
    state_posteriors: np.ndarray
    log_likelihoods: np.ndarray
    map_states: np.ndarray = None
    category_posteriors: np.ndarray = None
    pattern_rates: np.ndarray = None
    tip_posteriors: np.ndarray = None


@dataclass
class SprScan:
    """What Engine.spr_scan returns, with E = 2n-3 edges (edge e: the branch above node e): the
    trees' log-likelihoods [T]; per (tree, pruned edge s, direction) the target edge of the
    largest log-likelihood change best_target [T][E][2] (int32, -1: no move) and that change
    best_delta [T][E][2] (-inf: no move); best_move [T][3] = (s, direction, f) of the tree's
    largest change ((-1, -1, -1): none); on request delta [T][E][2][E], the whole table, -inf
    where (s, direction, f) is no move within the radius."""
    log_likelihoods: np.ndarray
    best_target: np.ndarray
    best_delta: np.ndarray
    best_move: np.ndarray
    delta: np.ndarray = None


@dataclass
class Placement:
    """What Engine.placement returns: the trees' log-likelihoods [T], per (tree, query, edge) the
    log-likelihood of the query on the edge's midpoint at the best of the pendant lengths
    edge_log_likelihoods [T][Q][2n-3] (edge e: the branch above node e) and best_edge [T][Q]
    (int32, the lowest among equals); on request pendant_index [T][Q][2n-3] (int8: which pendant
    length), lwr [T][Q][2n-3] (likelihood weight ratios, rows sum to 1) and tables
    [T][2n-3][G][5][P] (per edge, pendant length and pattern the log-likelihood of "the query shows
    A / C / G / T / gap")."""
    log_likelihoods: np.ndarray
    edge_log_likelihoods: np.ndarray
    best_edge: np.ndarray
    pendant_index: np.ndarray = None
    lwr: np.ndarray = None
    tables: np.ndarray = None


def rell_weights(weights, replicates, seed):
    """Replicate weights of a RELL bootstrap: multinomial resampling of sum(weights) sites over
    the patterns with numpy.random.default_rng(seed).  Returns float64 [replicates][P]; host
    arithmetic only.  Pattern weights that are no site counts (non-integer) are refused."""
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.size == 0 or not np.all(np.isfinite(w)) or np.any(w < 0) or np.any(w != np.rint(w)):
        raise RuntimeError("rell_weights: pattern weights must be non-negative integer site counts")
    total = int(w.sum())
    if total <= 0:
        raise RuntimeError("rell_weights: the pattern weights sum to 0")
    rng = np.random.default_rng(seed)
    return rng.multinomial(total, w / w.sum(), size=int(replicates)).astype(np.float64)


def _search_options(o, max_moves, pack_active, min_gain, branch_opt):
    """The fields that _capi.NniSearchOptions and _capi.SprSearchOptions share, into `o`."""
    o.max_moves, o.pack_active, o.min_gain = int(max_moves), int(bool(pack_active)), float(min_gain)
    if branch_opt:  # (left at zeros: the optimiser's defaults)
        keys = dict(max_iterations=100, check_interval=4, pack_active=True, tolerance=1e-6,
                    min_length=1e-8, max_length=10.0)
        unknown = set(branch_opt) - set(keys)
        if unknown:
            raise RuntimeError(f"unknown branch_opt options: {sorted(unknown)}")
        keys.update(branch_opt)
        o.branch_opt = _branch_opt_options(**keys)
    return o


def _nni_search_options(max_moves, pack_active, min_gain, branch_opt):
    return _search_options(_capi.NniSearchOptions(), max_moves, pack_active, min_gain, branch_opt)


def _spr_search_options(max_moves, pack_active, min_gain, radius, branch_opt):
    o = _search_options(_capi.SprSearchOptions(), max_moves, pack_active, min_gain, branch_opt)
    o.radius = int(radius)
    return o


def nni_neighbour(taxon_count, parent_ids, branch_lengths, node, which):
    """Neighbour `which` (0 | 1) of inner edge `node` of one unrooted tree (mi_nni_neighbour:
    the trees Engine.nni_scan scores): (parent ids [2n-3], branch lengths [2n-2]) renumbered
    in the reference's convention.  Host arithmetic only."""
    n = int(taxon_count)
    pid = _np(parent_ids, np.int32).reshape(2 * n - 3)
    bl = _np(branch_lengths, np.float64).reshape(2 * n - 2)
    out_pid, out_bl = np.empty(2 * n - 3, np.int32), np.empty(2 * n - 2)
    if _capi.load().mi_nni_neighbour(n, _ptr(pid), _ptr(bl), int(node), int(which), _ptr(out_pid),
                                     _ptr(out_bl)):
        raise RuntimeError(_capi.last_error())
    return out_pid, out_bl


def spr_neighbour(taxon_count, parent_ids, branch_lengths, s, direction, f):
    """The tree the SPR move (s, direction, f) of one unrooted tree leads to (mi_spr_neighbour:
    the trees Engine.spr_scan scores): (parent ids [2n-3], branch lengths [2n-2]) renumbered in
    the reference's convention.  Host arithmetic only."""
    n = int(taxon_count)
    pid = _np(parent_ids, np.int32).reshape(2 * n - 3)
    bl = _np(branch_lengths, np.float64).reshape(2 * n - 2)
    out_pid, out_bl = np.empty(2 * n - 3, np.int32), np.empty(2 * n - 2)
    if _capi.load().mi_spr_neighbour(n, _ptr(pid), _ptr(bl), int(s), int(direction), int(f), _ptr(out_pid),
                                     _ptr(out_bl)):
        raise RuntimeError(_capi.last_error())
    return out_pid, out_bl


@dataclass
class SplitTable:
    """Engine.split_index: the distinct splits of a batch of unrooted trees, numbered by first
    occurrence in (tree, edge) order (include/mi_phylo.h)."""
    taxon_count: int
    split_index: np.ndarray   # [T][2n-1] int32: index of edge v's split; -1 in entries 2n-3, 2n-2
    bits: np.ndarray          # [S][W] uint32: taxon i is bit i & 31 of word i >> 5; never taxon 0
    first: np.ndarray         # [S] entry number t (2n-1) + v of the first occurrence
    trees: np.ndarray         # [S] number of trees that hold the split
    stats: np.ndarray         # [S][3] sum w, sum w l, sum w l^2 over those trees, in tree order

    @property
    def split_count(self):
        return int(self.bits.shape[0])


def split_strings(bits, taxon_count):
    """The reference's "01110" form of stored splits (Bitset::ToString: taxon 0 first)."""
    n = int(taxon_count)
    b = _np(bits, np.uint32).reshape(-1, (n + 31) // 32)
    return ["".join("1" if (int(row[i >> 5]) >> (i & 31)) & 1 else "0" for i in range(n)) for row in b]


@dataclass
class SbnSupport:
    """Engine.sbn_index: the subsplit support of trees 0 .. support_tree_count-1 of a batch with
    its parameter numbering, and the slots of every tree of the batch (include/mi_phylo.h)."""
    taxon_count: int
    parent_ids: np.ndarray     # [T][2n-3] the batch
    support_tree_count: int
    root_index: np.ndarray     # [T][2n-3] parameter index of edge v's rootsplit, or P
    slot_index: np.ndarray     # [T][2(2n-3)][3] -1: no such slot; P: outside the support
    split_bits: np.ndarray     # [S][W] the rootsplits, as SplitTable.bits
    pcsp_clades: np.ndarray    # [C][3] sister, focal, child of PCSP S + i, each 2 split + side
    parent_range: np.ndarray   # [parents][2] parameter range [begin, end) of every block
    pcsp_parent: np.ndarray    # [C] block of PCSP S + i

    @property
    def rootsplit_count(self):
        return int(self.split_bits.shape[0])

    @property
    def pcsp_count(self):
        return int(self.pcsp_clades.shape[0])

    @property
    def parent_count(self):
        return int(self.parent_range.shape[0])

    @property
    def parameter_count(self):
        return self.rootsplit_count + self.pcsp_count


def _clade_strings(support):
    """"01110" of clade 2 split + side, for every clade the PCSPs name."""
    n = support.taxon_count
    plain = split_strings(support.split_bits, n)
    flip = ["".join("1" if c == "0" else "0" for c in s) for s in plain]
    return lambda clade: (flip if clade & 1 else plain)[clade >> 1]


def sbn_strings(support):
    """The reference's pretty indexer of a support (PrettyIndexer): "01110" for a rootsplit,
    "00001|11110|01110" (sister|focal|child) for a PCSP, in parameter order."""
    name = _clade_strings(support)
    return split_strings(support.split_bits, support.taxon_count) + \
        ["|".join(name(int(c)) for c in row) for row in support.pcsp_clades]


def sbn_rooted_representations(support, t):
    """Tree t's slots expanded to the reference's per-rooting index lists
    (UnrootedSBNMaps::IndexerRepresentationOf): [2n-3] lists, the rootsplit first.  A host helper
    for tests and small n: it walks the tree once per slot."""
    pid = [int(p) for p in support.parent_ids[t]]
    E = len(pid)
    kids = [[] for _ in range(E + 1)]
    for v in range(E):
        kids[pid[v]].append(v)
    slot = support.slot_index[t].reshape(2 * E, 3)
    out = [[int(support.root_index[t][v])] for v in range(E)]

    def below(v):  # the edges of the clade below v, its own included
        edges, stack = [], [v]
        while stack:
            x = stack.pop()
            edges.append(x)
            stack.extend(kids[x])
        return edges

    def above(v):  # the edges on the other side of node pid[v], the edge above it included
        p, edges = pid[v], []
        for c in kids[p]:
            if c != v:
                edges += below(c)
        return edges if p == E else edges + [p] + above(p)

    for v in range(E):
        p = pid[v]
        # the two other neighbours of p: the regions beyond them
        if p == E:
            x, y = [c for c in kids[p] if c != v]
            beyond = [below(x), below(y)]
        else:
            x = [c for c in kids[p] if c != v][0]
            beyond = [below(x), [p] + above(p)]
        for s in (0, 1):
            d = 2 * v + s
            if slot[d][0] >= 0:
                out[v].append(int(slot[d][0]))
            regions = beyond if s == 0 else ([below(c) for c in kids[v]] if kids[v] else [])
            for k in (1, 2):
                if slot[d][k] >= 0:
                    # the sister lies toward region k-1: the rootings in the other region use it
                    for edge in regions[2 - k]:
                        out[edge].append(int(slot[d][k]))
    return out


@dataclass
class PspTable:
    """Engine.psp_table: the PSP numbering of a support (include/mi_phylo.h).  The variables of a
    branch-length model are 0 .. variable_count-1: the rootsplits, then the PSPs."""
    psp_of_pcsp: np.ndarray    # [C] the variable of PCSP S + i if it is a PSP, else -1
    rootsplit_count: int       # S (the reference's after_rootsplits_index)
    variable_count: int        # V (the reference's first_empty_index): also the "not present" index


@dataclass
class BranchModelSample:
    """Engine.branch_model_sample: one draw of every particle's branch lengths."""
    branch_lengths: np.ndarray  # [T][2n-2] theta; entry 2n-3 is 0 (what the likelihood calls take)
    epsilon: np.ndarray         # [T][2n-3] the standard normals behind them
    log_q: np.ndarray           # [T] log q of the lengths
    log_prior: np.ndarray       # [T] the exponential prior


def psp_strings(support, table):
    """The reference's PSPIndexer::ToStringVector in this numbering: "01110" for a rootsplit,
    "focal|child" for a PSP, "" for the "not present" index variable_count (the last entry)."""
    name = _clade_strings(support)
    out = split_strings(support.split_bits, support.taxon_count) + [""] * (table.variable_count - table.rootsplit_count + 1)
    for row, j in zip(support.pcsp_clades, table.psp_of_pcsp):
        if j >= 0:
            out[int(j)] = name(int(row[1])) + "|" + name(int(row[2]))
    return out


def lognormal_mode_match(split_modes, table):
    """The reference's mode-matching heuristic (LogNormalModel.mode_match, PSPModel.mode_match) as
    q_params [V][2]: for split j with mode m_j, sigma = -0.1 log(clip(m, 1e-6, 1 - 1e-6)) and
    mu = sigma^2 + log(max(m, 1e-6)); the PSP rows are zero.  split_modes [S]: for instance the mean
    lengths stats[:, 1] / stats[:, 0] of Engine.split_index over the support's trees, whose
    numbering is the rootsplits'."""
    modes = _np(split_modes, np.float64).reshape(table.rootsplit_count)
    q = np.zeros((table.variable_count, 2))
    q[:table.rootsplit_count, 1] = -0.1 * np.log(np.clip(modes, 1e-6, 1 - 1e-6))
    q[:table.rootsplit_count, 0] = np.square(q[:table.rootsplit_count, 1]) + np.log(np.clip(modes, 1e-6, None))
    return q


def consensus_tree(taxon_count, split_bits, split_weight, total_weight, threshold=0.5):
    """The majority-rule consensus tree of a split table (mi_consensus_tree: host arithmetic
    only): every nontrivial split with weight > threshold * total_weight, threshold in
    [0.5, 1).  Returns (parent ids [m-1], node split [m]: the table index of each node's edge,
    -1 for the root), m = n+1 .. 2n-2 nodes in the reference's convention."""
    n = int(taxon_count)
    b = _np(split_bits, np.uint32).reshape(-1, (n + 31) // 32)
    w = _np(split_weight, np.float64).reshape(b.shape[0])
    m = C.c_int32()
    pid, node_split = np.empty(2 * n - 3, np.int32), np.empty(2 * n - 2, np.int32)
    if _capi.load().mi_consensus_tree(n, b.shape[0], _ptr(b), _ptr(w), float(total_weight), float(threshold),
                                      C.byref(m), _ptr(pid), _ptr(node_split)):
        raise RuntimeError(_capi.last_error())
    return pid[:m.value - 1].copy(), node_split[:m.value].copy()


def _parse_site(site):
    # src/site_model.cpp:10-25
    if site == "constant":
        return 0, 1
    if site.startswith("weibull"):
        idx = site.find("+")
        return 1, (int(site[idx + 1:]) if idx >= 0 else 4)
    raise RuntimeError("Site model not known: " + site)


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


_SBN_FACTORS = {"plain": 0, "vimco": 1, "given": 2}   # MI_SBN_FACTORS_*


def _sbn_factors(estimator):
    if estimator not in _SBN_FACTORS:
        raise RuntimeError(f"sbn_topology_gradient: estimator must be 'plain', 'vimco' or 'given', got {estimator!r}")
    return _SBN_FACTORS[estimator]


class Engine:
    """One MI355X engine: tips + pattern weights resident in HBM."""

    def __init__(self, model_specification, patterns, weights, use_tip_states=True,
                 device=-1, thread_count=1, tip_partials=None, reversible_model=None,
                 shard_devices=None, shard_mode="trees", device_tips=None):
        """patterns: [taxon][pattern] compact states (SitePattern::GetPatterns), or None when
        tip_partials ([taxon][pattern][s], SitePattern::GetPartials) is given with
        use_tip_states=False.  Substitution "WAG" / "reversible" makes a 20-state engine
        (s = 20); reversible_model = (exchangeabilities[190], frequencies[20]) replaces the
        built-in WAG table.  shard_devices (a list of HIP device ordinals, repeats allowed)
        makes ONE handle that drives several devices / logical shards
        (mi_engine_create_sharded): shard_mode "trees" deals the trees of a call in
        contiguous blocks, "patterns" gives every shard a block of site patterns and adds
        the per-tree results (unrooted calls).  Such a handle serves the numpy entry points;
        the *_device ones need one engine per device.  device_tips = (device pointer of the
        int32 [taxon][pattern] states, device pointer of the float64 weights, taxon count,
        pattern count) makes the engine from tips that are on the device already
        (mi_engine_create_device_tips; e.g. what site_pattern_compress_device(...,
        keep_on_device=True) hands out): patterns / weights are then None."""
        if thread_count == 0:  # src/engine.cpp:14-16
            raise RuntimeError("Thread count needs to be strictly positive.")
        self._lib = _capi.load()
        self._h = None
        if model_specification.substitution not in SUBST:
            raise RuntimeError("Substitution model not known: " +
                               model_specification.substitution)
        if model_specification.clock not in CLOCK:
            raise RuntimeError("Clock model not known: " + model_specification.clock)
        site_kind, K = _parse_site(model_specification.site)
        states = 20 if SUBST[model_specification.substitution] == 2 else 4
        self.state_count = states
        if device_tips is not None:
            # (this branch used to return before any validation and silently ignored
            # what does not combine with device-resident tips)
            for name, val in (("patterns", patterns), ("weights", weights), ("tip_partials", tip_partials),
                              ("reversible_model", reversible_model), ("shard_devices", shard_devices)):
                if val is not None:
                    raise RuntimeError(f"device_tips does not combine with {name}: the tips and weights "
                                       "are the device arrays, a 20-state engine made this way uses "
                                       "the built-in WAG table, and a sharded handle uploads its tips "
                                       "from host arrays")
            d_states, d_weights, n, P = device_tips
            if not d_states or not d_weights or int(n) < 3 or int(P) < 1:
                raise RuntimeError("device_tips = (states pointer, weights pointer, taxon count >= 3, "
                                   "pattern count >= 1)")
            self.taxon_count, self.pattern_count, self.category_count = n, P, K
            self.node_count = 2 * n - 1
            self.spec = _capi.EngineSpec(n, P, states, K, SUBST[model_specification.substitution],
                                         site_kind, CLOCK[model_specification.clock],
                                         1 if use_tip_states else 0, device, 0)
            h = C.c_void_p()
            self._check(self._lib.mi_engine_create_device_tips(
                C.byref(self.spec), C.c_void_p(d_states), C.c_void_p(d_weights), C.byref(h)))
            self._h = h
            self.param_count = self._lib.mi_engine_param_count(h)
            self.is_gtr = model_specification.substitution == "GTR"
            self._weights = None
            return
        weights = _np(weights, np.float64)
        self._weights = weights
        if tip_partials is not None:
            tip_partials = _np(tip_partials, np.float64)
            n, P = tip_partials.shape[:2]
            if tip_partials.shape != (n, P, states):
                raise RuntimeError(f"tip partials must be [taxon][pattern][{states}]")
        if patterns is not None:
            patterns = _np(patterns, np.int32)
            n, P = patterns.shape
        if weights.shape != (P,):
            raise RuntimeError("pattern weights must have one entry per site pattern")
        self.taxon_count, self.pattern_count, self.category_count = n, P, K
        self.node_count = 2 * n - 1
        self.spec = _capi.EngineSpec(n, P, states, K, SUBST[model_specification.substitution],
                                     site_kind, CLOCK[model_specification.clock],
                                     1 if use_tip_states else 0, device, 0)
        h = C.c_void_p()
        ex = fr = None
        if reversible_model is not None:  # validated before ANY create call reads the arrays
            if states != 20:
                raise RuntimeError("reversible_model needs a 20-state substitution model")
            ex, fr = (_np(x, np.float64) for x in reversible_model)
            if ex.shape != (190,) or fr.shape != (20,):
                raise RuntimeError("reversible_model must be (exchangeabilities[190], "
                                   "frequencies[20])")
        if patterns is not None and patterns.size and int(patterns.max()) > states:
            # (compact states are 0..s-1, s = gap; a 20-state pattern matrix handed to a
            # 4-state engine -- or the reverse, caught below for DNA codes only by value --
            # would be read as another alphabet)
            raise RuntimeError(f"compact tip states exceed the {states}-state alphabet "
                               f"(largest code {int(patterns.max())})")
        if shard_devices is not None:
            devs = _np(shard_devices, np.int32)
            mode = {"trees": 0, "patterns": 1}[shard_mode]
            rc = self._lib.mi_engine_create_sharded(
                C.byref(self.spec), len(devs), devs.ctypes.data_as(_capi.I32P), mode, _ptr(ex),
                _ptr(fr), _ptr(patterns), _ptr(tip_partials), _ptr(weights), C.byref(h))
        elif states == 20:
            rc = self._lib.mi_engine_create_reversible(
                C.byref(self.spec), _ptr(ex), _ptr(fr), _ptr(patterns), _ptr(tip_partials),
                _ptr(weights), C.byref(h))
        else:
            rc = self._lib.mi_engine_create(C.byref(self.spec), _ptr(patterns),
                                            _ptr(tip_partials), _ptr(weights), C.byref(h))
        self._check(rc)
        self._h = h
        self.param_count = self._lib.mi_engine_param_count(h)
        self.is_gtr = model_specification.substitution == "GTR"

    def close(self):
        if self._h is not None:
            self._lib.mi_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(_capi.last_error())

    # Engine::GetPhyloModelBlockSpecification (src/engine.cpp:48-52)
    def block_specification(self):
        out = {}
        for i in range(self._lib.mi_engine_block_count(self._h)):
            name, start, length = C.c_char_p(), C.c_int32(), C.c_int32()
            self._check(self._lib.mi_engine_block(self._h, i, C.byref(name), C.byref(start),
                                                  C.byref(length)))
            out[name.value.decode()] = (start.value, length.value)
        return out

    def _params(self, params, T):
        pr = _np(params if params is not None else np.zeros((T, self.param_count)), np.float64)
        if pr.ndim == 1 and self.param_count:
            pr = pr.reshape(-1, self.param_count) if pr.size % self.param_count == 0 else pr
        if self.param_count == 0:
            pr = np.zeros((T, 0))
        if pr.shape != (T, self.param_count):
            # fat_beagle.hpp:138 / block_specification.cpp:72-81
            raise RuntimeError("We param_matrix needs as many rows as we have trees "
                               f"and {self.param_count} columns; got {pr.shape}.")
        return np.ascontiguousarray(pr)

    # ---- host-pointer path (numpy in, numpy out) -------------------------------
    def log_likelihoods(self, parent_ids, branch_lengths, params=None, rescaling=False):
        """Engine::LogLikelihoods(const UnrootedTreeCollection&, ...)."""
        n = self.taxon_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        if T == 0:  # FatBeagleParallelize over an empty collection returns an empty vector
            return np.empty(0)
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        out = np.empty(T)
        self._check(self._lib.mi_engine_log_likelihoods_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), _ptr(out)))
        return out

    def gradients(self, parent_ids, branch_lengths, params=None, rescaling=False,
                  gradient_blocks=None):
        """Engine::Gradients(const UnrootedTreeCollection&, ...) -> [PhyloGradient].

        gradient_blocks (an extension): None = every block the reference returns; or a
        collection of block names the caller will read ("branch_lengths" always comes) --
        a caller that only uses the branch-length gradient of a GTR model (vip does) saves
        the 16 finite-difference passes behind "substitution_model" and the extra pass
        behind "site_model"; what is returned is bit-identical to the full call."""
        n, N = self.taxon_count, self.node_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        if T == 0:
            return []
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        ll, g = np.empty(T), np.empty((T, N))
        want = None if gradient_blocks is None else set(gradient_blocks)
        site = np.empty(T) if want is None or "site_model" in want else None
        subst = np.empty((T, 8)) if want is None or "substitution_model" in want else None
        self._check(self._lib.mi_engine_gradients_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), _ptr(ll), _ptr(g),
            _ptr(site), _ptr(subst)))
        return self._phylo_gradients(ll, {"branch_lengths": g}, site, subst)

    def gradients_reduced(self, parent_ids, branch_lengths, params, branch_index, index_count,
                          tree_weights=None, rescaling=False):
        """One variational-inference step's reductions behind the gradient call
        (mi_engine_gradients_unrooted_reduced; vip/burrito.py:143-166,
        vip/branch_model.py:125-132): returns (sum_t w_t logL_t, sum_t w_t site gradient_t,
        index_gradient[index_count] = scatter-add of the branch gradients by branch_index
        (negative = skip), per-tree log-likelihoods)."""
        n, N = self.taxon_count, self.node_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        bi = _np(branch_index, np.int32).reshape(T, N)
        tw = None if tree_weights is None else _np(tree_weights, np.float64).reshape(T)
        sums, ig, ll = np.zeros(2), np.zeros(max(index_count, 1)), np.empty(T)
        self._check(self._lib.mi_engine_gradients_unrooted_reduced(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), _ptr(bi), _ptr(tw),
            int(index_count), _ptr(sums), _ptr(ig), _ptr(ll)))
        return sums[0], sums[1], ig[:index_count], ll

    def branch_hessian(self, parent_ids, branch_lengths, params=None, rescaling=False,
                       squared_gradient=False):
        """Diagonal of the branch-length Hessian per tree (mi_engine_branch_hessian_unrooted;
        an extension, 4-state engines): returns (log-likelihoods [T], branch gradient [T][2n-1],
        d^2 logL / d t_j^2 [T][2n-1]) and, with squared_gradient=True, also
        S [T][2n-1] = sum_p w_p (d log L_p / d t_j)^2.  Root and fixed node entries are 0."""
        n, N = self.taxon_count, self.node_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        if T == 0:
            empty = (np.empty(0), np.empty((0, N)), np.empty((0, N)))
            return empty + ((np.empty((0, N)),) if squared_gradient else ())
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        ll, g, h = np.empty(T), np.empty((T, N)), np.empty((T, N))
        s = np.empty((T, N)) if squared_gradient else None
        self._check(self._lib.mi_engine_branch_hessian_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), _ptr(ll), _ptr(g),
            _ptr(h), _ptr(s)))
        return (ll, g, h, s) if squared_gradient else (ll, g, h)

    def nni_scan(self, parent_ids, branch_lengths, params=None, rescaling=False):
        """Log-likelihood change of every nearest-neighbour interchange per tree
        (mi_engine_nni_scan_unrooted; an extension, 4-state engines): returns (log-likelihoods
        [T], delta [T][2n-1][2] by node id -- delta[t][v][i] = logL(neighbour i of inner edge v)
        - logL(tree t), 0 where v is no inner edge --, best move [T] = 2 v + i of the largest
        delta, -1 for three taxa).  nni_neighbour builds the tree a move leads to."""
        n, N = self.taxon_count, self.node_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        if T == 0:
            return np.empty(0), np.empty((0, N, 2)), np.empty(0, np.int32)
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        ll, delta, best = np.empty(T), np.empty((T, N, 2)), np.empty(T, np.int32)
        self._check(self._lib.mi_engine_nni_scan_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), _ptr(ll), _ptr(delta),
            _ptr(best)))
        return ll, delta, best

    def spr_scan(self, parent_ids, branch_lengths, params=None, rescaling=False, radius=0, table=False):
        """Log-likelihood change of every subtree-prune-and-regraft move per tree
        (mi_engine_spr_scan_unrooted; an extension, 4-state engines): move (s, direction, f) cuts
        edge s (direction 0: clade s moves, 1: the rest moves) and re-attaches the loose part on
        the midpoint of edge f.  radius 0 scans every move, radius r those at most r nodes from the
        prune point.  Returns an SprScan (table=True: with the whole table); spr_neighbour builds
        the tree a move leads to."""
        n = self.taxon_count
        E = 2 * n - 3
        pid = _np(parent_ids, np.int32).reshape(-1, E)
        T = pid.shape[0]
        ll, target, best = np.empty(T), np.empty((T, E, 2), np.int32), np.empty((T, E, 2))
        move = np.empty((T, 3), np.int32)
        delta = np.empty((T, E, 2, E)) if table else None
        if T:
            bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
            pr = self._params(params, T)
            self._check(self._lib.mi_engine_spr_scan_unrooted(
                self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), int(radius), _ptr(ll), _ptr(target),
                _ptr(best), _ptr(move), _ptr(delta)))
        return SprScan(ll, target, best, move, delta)

    def ancestral_states(self, parent_ids, branch_lengths, params=None, rescaling=False,
                         map_states=False, categories=False, tips=False):
        """Marginal ancestral-state posteriors per tree, internal node and pattern
        (mi_engine_ancestral_states_unrooted; an extension, 4-state engines): an AncestralStates
        with state_posteriors and log_likelihoods -- those of a gradient call on the HBM path,
        bit for bit -- and, asked for, map_states, category_posteriors with pattern_rates
        (categories=True) and tip_posteriors.  What is not asked for is not computed."""
        n, P, K = self.taxon_count, self.pattern_count, self.category_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        state, ll = np.empty((T, n - 2, P, 4)), np.empty(T)
        mp = np.empty((T, n - 2, P), np.int8) if map_states else None
        cat = np.empty((T, P, K)) if categories else None
        rate = np.empty((T, P)) if categories else None
        tip = np.empty((T, n, P, 4)) if tips else None
        if T:
            bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
            pr = self._params(params, T)
            self._check(self._lib.mi_engine_ancestral_states_unrooted(
                self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), _ptr(ll), _ptr(state),
                _ptr(mp), _ptr(cat), _ptr(rate), _ptr(tip)))
        return AncestralStates(state, ll, mp, cat, rate, tip)

    def placement(self, parent_ids, branch_lengths, queries, pendant_lengths, params=None, rescaling=False,
                  column_pattern=None, column_weights=None, pendant_index=False, lwr=False, tables=False):
        """Phylogenetic placement (mi_engine_placement_unrooted; an extension, 4-state engines):
        every query row of `queries` [Q][C] (compact states 0..3, anything else a gap) scored on
        the midpoint of every edge of every tree, at each of the 1..4 pendant_lengths.
        column_pattern [C] names the engine pattern each query column extends and column_weights
        [C] weighs it (None: 1); column_pattern=None means C = P, the identity map and the
        engine's pattern weights.  Returns a Placement; what is not asked for is not computed."""
        n, P = self.taxon_count, self.pattern_count
        E = 2 * n - 3
        pid = _np(parent_ids, np.int32).reshape(-1, E)
        T = pid.shape[0]
        x = _np(queries, np.int8)
        if x.ndim != 2:
            raise RuntimeError("queries must be [query][column]")
        Q, Cn = x.shape
        if column_pattern is None:
            if column_weights is None:
                if self._weights is None:
                    raise RuntimeError("an engine made from device tips keeps no pattern weights on the host: "
                                       "pass column_pattern and column_weights")
                column_weights = self._weights
            col = np.arange(P, dtype=np.int32)
        else:
            col = _np(column_pattern, np.int32).reshape(-1)
        if col.shape != (Cn,):
            raise RuntimeError(f"queries have {Cn} columns, the column map {col.shape[0]}")
        cw = None
        if column_weights is not None:
            cw = _np(column_weights, np.float64).reshape(-1)
            if cw.shape != (Cn,):
                raise RuntimeError("column_weights must have one entry per query column")
        pend = _np(pendant_lengths, np.float64).reshape(-1)
        G = pend.shape[0]
        ll, edge = np.empty(T), np.empty((T, Q, E))
        best = np.empty((T, Q), np.int32)
        pi = np.empty((T, Q, E), np.int8) if pendant_index else None
        lw = np.empty((T, Q, E)) if lwr else None
        tab = np.empty((T, E, G, 5, P)) if tables else None
        if T:
            bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
            pr = self._params(params, T)
            self._check(self._lib.mi_engine_placement_unrooted(
                self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), Q, Cn, _ptr(x), _ptr(col), _ptr(cw),
                G, _ptr(pend), _ptr(ll), _ptr(edge), _ptr(pi), _ptr(best), _ptr(lw), _ptr(tab)))
        return Placement(ll, edge, best, pi, lw, tab)

    def pattern_log_likelihoods(self, parent_ids, branch_lengths, params=None, rescaling=False):
        """Per-pattern log-likelihoods per tree (mi_engine_pattern_log_likelihoods_unrooted; an
        extension, 4-state engines): returns (log-likelihoods [T] -- what log_likelihoods returns,
        bit for bit --, log L_p [T][P], unweighted; a pattern of likelihood 0 gives -inf)."""
        n, P = self.taxon_count, self.pattern_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        if T == 0:
            return np.empty(0), np.empty((0, P))
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        ll, s = np.empty(T), np.empty((T, P))
        self._check(self._lib.mi_engine_pattern_log_likelihoods_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), _ptr(ll), _ptr(s)))
        return ll, s

    def rell(self, pattern_log_likelihoods, replicate_weights, replicate_log_likelihoods=True):
        """RELL re-summation (mi_engine_rell): s [T][P], W [B][P] -> (C [B][T] = W s^T or None,
        best tree [B], bootstrap proportions [T], expected-likelihood weights [T]).  Any engine
        serves: P is the matrices'.  replicate_log_likelihoods=False: C stays on the device."""
        s = _np(pattern_log_likelihoods, np.float64)
        w = _np(replicate_weights, np.float64)
        if s.ndim != 2 or w.ndim != 2 or s.shape[1] != w.shape[1]:
            raise RuntimeError("rell: pattern log-likelihoods [T][P] and replicate weights [B][P] "
                               f"must share P; got {s.shape} and {w.shape}")
        (T, P), B = s.shape, w.shape[0]
        c = np.empty((B, T)) if replicate_log_likelihoods else None
        best, bp, elw = np.empty(B, np.int32), np.empty(T), np.empty(T)
        self._check(self._lib.mi_engine_rell(self._h, B, T, P, _ptr(s), _ptr(w), _ptr(c), _ptr(best),
                                             _ptr(bp), _ptr(elw)))
        return c, best, bp, elw

    def rell_bootstrap(self, parent_ids, branch_lengths, replicate_weights, params=None,
                       rescaling=False):
        """Per-pattern log-likelihoods and their RELL re-summation in one host call
        (mi_engine_rell_bootstrap_unrooted; single-device 4-state engines): replicate_weights
        [B][P] (rell_weights makes them).  Returns a RellResult."""
        n, P = self.taxon_count, self.pattern_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        w = _np(replicate_weights, np.float64)
        if w.ndim != 2 or w.shape[1] != P:
            raise RuntimeError(f"replicate weights must be [B][{P}]; got {w.shape}")
        B = w.shape[0]
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        out = RellResult(np.empty(T), np.empty((T, P)), np.empty((B, T)), np.empty(B, np.int32),
                         np.empty(T), np.empty(T))
        self._check(self._lib.mi_engine_rell_bootstrap_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), B, _ptr(w),
            _ptr(out.log_likelihood), _ptr(out.pattern_log_likelihood),
            _ptr(out.replicate_log_likelihood), _ptr(out.best_tree), _ptr(out.bootstrap_proportion),
            _ptr(out.expected_likelihood_weight)))
        return out

    def bootstrap_weights(self, replicates, sites=None, seed=0, first_replicate=0, weights=None):
        """Replicate weights of a bootstrap drawn on the device (mi_engine_bootstrap_weights):
        `replicates` rows of `sites` draws each (default: N = sum of the weights, the ordinary
        bootstrap; another count: a scaled replicate of the AU test) over the patterns of
        `weights` (default: the engine's pattern weights; non-negative integer site counts).  A
        row's bits depend on (seed, first_replicate + row, sites, weights) alone.  Returns float64
        [replicates][P] in the layout rell, rell_bootstrap, pairwise_distances and starting_trees
        take as replicate_weights: it can be handed over as it is."""
        w = self._weights if weights is None else weights
        if w is None:
            raise RuntimeError("bootstrap_weights: this engine keeps no host copy of its pattern weights; "
                               "pass weights")
        w = _np(w, np.float64).reshape(-1)
        B = int(replicates)
        n = int(w.sum()) if sites is None else int(sites)
        out = np.empty((B, w.size))
        self._check(self._lib.mi_engine_bootstrap_weights(self._h, w.size, _ptr(w), B, n, int(seed),
                                                          int(first_replicate), _ptr(out)))
        return out

    def topology_tests_matrix(self, pattern_log_likelihoods, weights, sites, replicates, seed=0,
                              first_replicate=0, replicate_log_likelihoods=False):
        """The KH, SH and AU tests with BP and ELW from per-pattern log-likelihoods s [T][P] and
        pattern weights [P] (mi_engine_topology_tests; any engine serves): block k draws
        replicates[k] replicates of sites[k] sites on the device (sites[0] = N).  Returns a
        TopologyTests."""
        s = _np(pattern_log_likelihoods, np.float64)
        w = _np(weights, np.float64).reshape(-1)
        if s.ndim != 2 or s.shape[1] != w.size:
            raise RuntimeError("topology tests: pattern log-likelihoods [T][P] and pattern weights [P] "
                               f"must share P; got {s.shape} and {w.shape}")
        T, P = s.shape
        si, reps = _np(sites, np.int64).reshape(-1), _np(replicates, np.int32).reshape(-1)
        if si.size != reps.size or si.size < 1:
            raise RuntimeError("topology tests: sites and replicates must have one entry per block")
        K = si.size
        B0 = max(int(reps[0]), 0)
        table, counts, mean = np.empty((T, 11)), np.empty((K, T), np.int32), np.empty(T)
        c = np.empty((B0, T)) if replicate_log_likelihoods else None
        best = np.empty(B0, np.int32) if replicate_log_likelihoods else None
        self._check(self._lib.mi_engine_topology_tests(
            self._h, T, P, _ptr(s), _ptr(w), K, _ptr(si), _ptr(reps), int(seed), int(first_replicate),
            _ptr(table), _ptr(counts), _ptr(mean), _ptr(c), _ptr(best)))
        return TopologyTests.from_table(table, counts, mean, si, reps, c, best)

    def topology_tests(self, parent_ids, branch_lengths, params=None, rescaling=False,
                       scales=(1.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.1, 1.2, 1.3, 1.4), replicates=10000,
                       seed=0, first_replicate=0, replicate_log_likelihoods=False):
        """From trees to the table of p-values in one host call
        (mi_engine_topology_tests_unrooted; single-device 4-state engines): the per-pattern
        log-likelihoods, then the tests with the engine's own pattern weights, nothing returning
        to the host in between.  scales[0] must be 1; block k draws `replicates` (one count, or
        one per scale) replicates of floor(scales[k] N + 0.5) sites.  Returns a TopologyTests
        (with the per-pattern log-likelihoods)."""
        n, P = self.taxon_count, self.pattern_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        if self._weights is None:
            raise RuntimeError("topology_tests: this engine keeps no host copy of its pattern weights; use "
                               "pattern_log_likelihoods and topology_tests_matrix")
        N = int(np.rint(float(np.sum(self._weights))))
        sc = np.asarray(scales, np.float64).reshape(-1)
        si = np.floor(sc * N + 0.5).astype(np.int64)
        reps = np.ascontiguousarray(np.broadcast_to(np.asarray(replicates, np.int32), sc.shape))
        K = si.size
        if K < 1:
            raise RuntimeError("topology tests: at least one scale")
        B0 = max(int(reps[0]), 0)
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        ll, s = np.empty(T), np.empty((T, P))
        table, counts, mean = np.empty((T, 11)), np.empty((K, T), np.int32), np.empty(T)
        c = np.empty((B0, T)) if replicate_log_likelihoods else None
        best = np.empty(B0, np.int32) if replicate_log_likelihoods else None
        self._check(self._lib.mi_engine_topology_tests_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), K, _ptr(si), _ptr(reps), int(seed),
            int(first_replicate), _ptr(ll), _ptr(s), _ptr(table), _ptr(counts), _ptr(mean), _ptr(c), _ptr(best)))
        out = TopologyTests.from_table(table, counts, mean, si, reps, c, best)
        out.tree_log_likelihood, out.pattern_log_likelihood = ll, s
        return out

    def _replicates(self, replicate_weights):
        if replicate_weights is None:  # one replicate: the engine's pattern weights
            return None, 1
        w = _np(replicate_weights, np.float64)
        if w.ndim != 2 or w.shape[1] != self.pattern_count:
            raise RuntimeError(f"replicate weights must be [B][{self.pattern_count}]; got {w.shape}")
        return w, w.shape[0]

    def _model_row(self, params):
        if self.param_count == 0:
            return None
        if params is None:
            raise RuntimeError(f"the model needs one parameter row of {self.param_count} entries")
        pr = _np(params, np.float64).reshape(-1)
        if pr.shape != (self.param_count,):
            raise RuntimeError(f"pairwise distances take ONE parameter row of {self.param_count} "
                               f"entries; got {pr.shape}")
        return pr

    def pairwise_distances(self, replicate_weights=None, params=None, pair_counts=False,
                           pair_status=False, min_length=1e-8, max_length=10.0, tolerance=1e-10,
                           max_iterations=50):
        """Maximum-likelihood distances of all pairs of taxa (mi_engine_pairwise_distances; an
        extension, 4-state engines) for every row of replicate_weights [B][P] (None: the
        engine's pattern weights, B = 1) under ONE model row.  Returns a PairwiseDistances."""
        n = self.taxon_count
        w, B = self._replicates(replicate_weights)
        pr = self._model_row(params)
        opts = _distance_options(min_length, max_length, tolerance, max_iterations)
        pairs = n * (n - 1) // 2
        out = PairwiseDistances(np.empty((B, n, n)),
                                np.empty((B, pairs, 4, 4)) if pair_counts else None,
                                np.empty((B, pairs), np.int8) if pair_status else None)
        self._check(self._lib.mi_engine_pairwise_distances(
            self._h, B, _ptr(w), _ptr(pr), C.addressof(opts), _ptr(out.distances),
            _ptr(out.pair_counts), _ptr(out.pair_status)))
        return out

    def neighbour_joining(self, distances, min_length=1e-8, max_length=10.0):
        """Neighbour joining of distance matrices [B][n][n] (mi_engine_neighbour_joining; only
        i < j is read; any engine serves: n is the matrices').  Returns (parent ids [B][2n-3],
        branch lengths [B][2n-2], clamped into [min_length, max_length]) in the form every
        unrooted call takes."""
        d = _np(distances, np.float64)
        if d.ndim == 2:
            d = d[None]
        if d.ndim != 3 or d.shape[1] != d.shape[2] or d.shape[1] < 3 or d.shape[0] < 1:
            raise RuntimeError(f"neighbour joining takes distances [B][n][n], n >= 3; got {d.shape}")
        B, n = d.shape[:2]
        d = np.ascontiguousarray(d)
        pid, bl = np.empty((B, 2 * n - 3), np.int32), np.empty((B, 2 * n - 2))
        self._check(self._lib.mi_engine_neighbour_joining(
            self._h, B, n, _ptr(d), float(min_length), float(max_length), _ptr(pid), _ptr(bl)))
        return pid, bl

    def starting_trees(self, replicate_weights=None, params=None, distances=False, min_length=1e-8,
                       max_length=10.0, tolerance=1e-10, max_iterations=50):
        """Neighbour-joining trees of the maximum-likelihood distances in one host call
        (mi_engine_starting_trees_unrooted): pairwise_distances followed by neighbour_joining,
        bit for bit, nothing returning to the host in between.  Returns a StartingTrees."""
        n = self.taxon_count
        w, B = self._replicates(replicate_weights)
        pr = self._model_row(params)
        opts = _distance_options(min_length, max_length, tolerance, max_iterations)
        out = StartingTrees(np.empty((B, 2 * n - 3), np.int32), np.empty((B, 2 * n - 2)),
                            np.empty((B, n, n)) if distances else None)
        self._check(self._lib.mi_engine_starting_trees_unrooted(
            self._h, B, _ptr(w), _ptr(pr), C.addressof(opts), _ptr(out.parent_ids),
            _ptr(out.branch_lengths), _ptr(out.distances)))
        return out

    def split_index(self, parent_ids, branch_lengths=None, tree_weights=None, split_capacity=None):
        """The split table of a batch of unrooted trees [T][2n-3] (mi_engine_split_index; any
        engine serves: n is the trees').  branch_lengths [T][2n-2] and tree_weights [T] enter
        the statistics only.  split_capacity: rows of the table (default T (2n-3), which always
        suffices).  Returns a SplitTable."""
        pid = _np(parent_ids, np.int32)
        if pid.ndim == 1:
            pid = pid[None]
        if pid.ndim != 2 or pid.shape[0] < 1 or pid.shape[1] < 3 or pid.shape[1] % 2 == 0:
            raise RuntimeError(f"split_index takes parent ids [T][2n-3], n >= 3; got {pid.shape}")
        T, E = pid.shape
        n = (E + 3) // 2
        bl = None if branch_lengths is None else _np(branch_lengths, np.float64).reshape(T, E + 1)
        tw = None if tree_weights is None else _np(tree_weights, np.float64).reshape(T)
        cap = T * E if split_capacity is None else int(split_capacity)
        W = (n + 31) // 32
        index, count = np.empty((T, E + 2), np.int32), np.zeros(1, np.int32)
        bits, first, trees = np.zeros((cap, W), np.uint32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        stats = np.zeros((cap, 3))
        self._check(self._lib.mi_engine_split_index(
            self._h, T, n, _ptr(pid), _ptr(bl), _ptr(tw), cap, _ptr(index), _ptr(count), _ptr(bits),
            _ptr(first), _ptr(trees), _ptr(stats)))
        S = int(count[0])
        return SplitTable(n, index, bits[:S].copy(), first[:S].copy(), trees[:S].copy(), stats[:S].copy())

    def sbn_index(self, parent_ids, support_tree_count=None, rootsplit_capacity=None, pcsp_capacity=None):
        """The subsplit support of a batch of unrooted trees [T][2n-3] and every tree's slots
        (mi_engine_sbn_index; any engine serves).  The support is that of the first
        support_tree_count trees (default: all); the later ones are only looked up and get the
        sentinel P where they leave it.  Capacities default to what always suffices.  Returns an
        SbnSupport."""
        pid = _np(parent_ids, np.int32)
        if pid.ndim == 1:
            pid = pid[None]
        if pid.ndim != 2 or pid.shape[0] < 1 or pid.shape[1] < 3 or pid.shape[1] % 2 == 0:
            raise RuntimeError(f"sbn_index takes parent ids [T][2n-3], n >= 3; got {pid.shape}")
        T, E = pid.shape
        n = (E + 3) // 2
        T0 = T if support_tree_count is None else int(support_tree_count)
        rcap = max(T0, 1) * E if rootsplit_capacity is None else int(rootsplit_capacity)
        pcap = max(T0, 1) * E * 6 if pcsp_capacity is None else int(pcsp_capacity)
        W = (n + 31) // 32
        root, slot = np.empty((T, E), np.int32), np.empty((T, 2 * E, 3), np.int32)
        counts = np.zeros(3, np.int32)
        bits, clades = np.zeros((rcap, W), np.uint32), np.zeros((pcap, 3), np.int32)
        prange, parent = np.zeros((pcap, 2), np.int32), np.zeros(pcap, np.int32)
        self._check(self._lib.mi_engine_sbn_index(
            self._h, T, n, _ptr(pid), T0, rcap, pcap, _ptr(root), _ptr(slot), _ptr(counts), _ptr(bits),
            _ptr(clades), _ptr(prange), _ptr(parent)))
        S, Cn, parents = (int(x) for x in counts)
        return SbnSupport(n, pid.copy(), T0, root, slot, bits[:S].copy(), clades[:Cn].copy(),
                          prange[:parents].copy(), parent[:Cn].copy())

    def _sbn_trees(self, support, trees):
        """(parent ids, root index, slot index) of `trees`: None (the support's own batch), a
        range / index array into it, or an SbnSupport indexed against the same support."""
        if trees is None:
            return support.parent_ids, support.root_index, support.slot_index
        if isinstance(trees, SbnSupport):
            return trees.parent_ids, trees.root_index, trees.slot_index
        idx = np.arange(support.parent_ids.shape[0])[trees]
        return (np.ascontiguousarray(support.parent_ids[idx]), np.ascontiguousarray(support.root_index[idx]),
                np.ascontiguousarray(support.slot_index[idx]))

    def sbn_log_prob(self, support, log_params, trees=None, normalized=False, tree_weights=None,
                     expected_counts=False):
        """log p of every rooting [T][2n-3] and log q [T] of trees of a support's batch under
        log_params [P] (mi_engine_sbn_log_prob); with expected_counts also
        log sum_t w_t usage_t [P] (the E-step).  trees: see _sbn_trees."""
        pid, root, slot = self._sbn_trees(support, trees)
        T, E = pid.shape
        P = support.parameter_count
        th = _np(log_params, np.float64).reshape(P)
        tw = None if tree_weights is None else _np(tree_weights, np.float64).reshape(T)
        lp, lq = np.empty((T, E)), np.empty(T)
        counts = np.empty(P) if expected_counts else None
        self._check(self._lib.mi_engine_sbn_log_prob(
            self._h, T, support.taxon_count, _ptr(pid), _ptr(root), _ptr(slot), support.rootsplit_count,
            support.pcsp_count, support.parent_count, _ptr(support.parent_range), _ptr(th), int(bool(normalized)),
            _ptr(tw), _ptr(lp), _ptr(lq), _ptr(counts)))
        return (lp, lq, counts) if expected_counts else (lp, lq)

    def sbn_normalize(self, support, log_params):
        """Log-normalise log_params [P] over the rootsplits and every parent's block
        (mi_engine_sbn_normalize)."""
        P = support.parameter_count
        th, out = _np(log_params, np.float64).reshape(P), np.empty(P)
        self._check(self._lib.mi_engine_sbn_normalize(
            self._h, support.rootsplit_count, support.pcsp_count, support.parent_count,
            _ptr(support.parent_range), _ptr(th), _ptr(out)))
        return out

    def sbn_train(self, support, method="sa", tree_weights=None, alpha=0.0, max_iter=0, score_epsilon=0.0,
                  trees=None):
        """Simple-average ("sa") or EM ("em") training on trees of a support's batch (default: its
        support trees) with topology counts tree_weights (mi_engine_sbn_train).  Returns
        (normalised log parameters [P], score history [iterations])."""
        if method not in ("sa", "em"):
            raise RuntimeError(f"sbn_train: method must be 'sa' or 'em', got {method!r}")
        pid, root, slot = self._sbn_trees(support, slice(0, support.support_tree_count) if trees is None else trees)
        T = pid.shape[0]
        P = support.parameter_count
        tw = None if tree_weights is None else _np(tree_weights, np.float64).reshape(T)
        out, history, iters = np.empty(P), np.zeros(max(int(max_iter), 1)), np.zeros(1, np.int32)
        self._check(self._lib.mi_engine_sbn_train(
            self._h, T, support.taxon_count, _ptr(pid), _ptr(root), _ptr(slot), support.rootsplit_count,
            support.pcsp_count, support.parent_count, _ptr(support.parent_range), _ptr(tw),
            0 if method == "sa" else 1, float(alpha), int(max_iter), float(score_epsilon), _ptr(out),
            _ptr(history), _ptr(iters)))
        return out, history[:int(iters[0])].copy()

    def sbn_descent(self, support):
        """The descent table [P][2] of a support (mi_engine_sbn_descent): the two parent subsplits
        every parameter leads to, >= 0 a block of parent_range, < 0 the leaf ~value."""
        T0 = support.support_tree_count
        pid = np.ascontiguousarray(support.parent_ids[:T0])
        root = np.ascontiguousarray(support.root_index[:T0])
        slot = np.ascontiguousarray(support.slot_index[:T0])
        out = np.empty((support.parameter_count, 2), np.int32)
        self._check(self._lib.mi_engine_sbn_descent(
            self._h, T0, support.taxon_count, _ptr(pid), _ptr(root), _ptr(slot), support.rootsplit_count,
            support.pcsp_count, _ptr(support.pcsp_parent), _ptr(out)))
        return out

    def sbn_sample(self, support, descent, log_params, K, seed, first_sample=0, cdf=False):
        """K topologies drawn from the SBN with (unnormalised) log_params [P] by the Philox stream
        (seed, first_sample + k) (mi_engine_sbn_sample).  Returns (parent ids [K][2n-3], root edge
        [K], sampled parameters [K][n-1], log probability [K]), with cdf=True also the CDF [P]."""
        n, P, K = support.taxon_count, support.parameter_count, int(K)
        th = _np(log_params, np.float64).reshape(P)
        desc = _np(descent, np.int32).reshape(P, 2)
        pid, edge = np.empty((K, 2 * n - 3), np.int32), np.empty(K, np.int32)
        params, lp = np.empty((K, n - 1), np.int32), np.empty(K)
        out_cdf = np.empty(P) if cdf else None
        self._check(self._lib.mi_engine_sbn_sample(
            self._h, K, n, support.rootsplit_count, support.pcsp_count, support.parent_count,
            _ptr(support.parent_range), _ptr(desc), _ptr(th), int(seed) & (2 ** 64 - 1), int(first_sample),
            _ptr(pid), _ptr(edge), _ptr(params), _ptr(lp), _ptr(out_cdf)))
        return (pid, edge, params, lp, out_cdf) if cdf else (pid, edge, params, lp)

    def sbn_topology_gradient(self, support, log_params, log_f, estimator="vimco", trees=None, normalized=False):
        """The gradient of the multi-sample variational objective with respect to the unnormalised
        SBN parameters (mi_engine_sbn_topology_gradient) for trees of a support's batch (see
        _sbn_trees) with log_f [K]; estimator "plain", "vimco" or "given" (log_f holds the
        factors).  Returns (gradient [P], factors [K], log q [K])."""
        code = _sbn_factors(estimator)
        pid, root, slot = self._sbn_trees(support, trees)
        T = pid.shape[0]
        P = support.parameter_count
        th, f = _np(log_params, np.float64).reshape(P), _np(log_f, np.float64).reshape(T)
        grad, factors, lq = np.empty(P), np.empty(T), np.empty(T)
        self._check(self._lib.mi_engine_sbn_topology_gradient(
            self._h, T, support.taxon_count, _ptr(pid), _ptr(root), _ptr(slot), support.rootsplit_count,
            support.pcsp_count, support.parent_count, _ptr(support.parent_range), _ptr(th), int(bool(normalized)),
            _ptr(f), code, _ptr(grad), _ptr(factors), _ptr(lq)))
        return grad, factors, lq

    def psp_table(self, support):
        """The PSP numbering of a support (mi_engine_psp_table).  Returns a PspTable."""
        S, Cn = support.rootsplit_count, support.pcsp_count
        clades = _np(support.pcsp_clades, np.int32).reshape(Cn, 3)
        out, counts = np.empty(Cn, np.int32), np.zeros(2, np.int32)
        self._check(self._lib.mi_engine_psp_table(self._h, S, Cn, _ptr(clades) if Cn else None,
                                                  _ptr(out) if Cn else None, _ptr(counts)))
        return PspTable(out, int(counts[0]), int(counts[1]))

    def psp_index(self, support, table, rows=3, trees=None):
        """The index rows [T][rows][2n-3] of trees of a support's batch (mi_engine_psp_index; trees
        as _sbn_trees): row 0 the split of every edge, with rows=3 also its down and its up PSP;
        table.variable_count where there is none."""
        _, root, slot = self._sbn_trees(support, trees)
        T, E = root.shape
        out = np.empty((T, int(rows), E), np.int32)
        Cn = support.pcsp_count
        psp = _np(table.psp_of_pcsp, np.int32).reshape(Cn)
        self._check(self._lib.mi_engine_psp_index(
            self._h, T, support.taxon_count, _ptr(root), _ptr(slot), support.rootsplit_count, Cn,
            _ptr(psp) if Cn else None, table.variable_count, int(rows), _ptr(out)))
        return out

    @staticmethod
    def _branch_model_shape(index, q_params):
        idx = _np(index, np.int32)
        if idx.ndim != 3 or idx.shape[2] < 3 or idx.shape[2] % 2 == 0:
            raise RuntimeError(f"the branch-length models take an index [T][rows][2n-3]; got {idx.shape}")
        q = _np(q_params, np.float64)
        if q.ndim != 2 or q.shape[1] != 2:
            raise RuntimeError(f"the branch-length models take q_params [V][2]; got {q.shape}")
        return idx, q, idx.shape[0], idx.shape[1], idx.shape[2]

    def branch_model_sample(self, index, q_params, seed, first_sample=0, prior_rate=10.0, epsilon=None):
        """Branch lengths of T particles drawn from the log-normal q with (mu, sigma) tables
        q_params [V][2] summed over index [T][rows][2n-3] (Engine.psp_index), log q and the
        exponential prior (mi_engine_branch_model_sample).  Particle t takes the Philox stream
        (seed, first_sample + t), or epsilon [T][2n-3] if given.  Returns a BranchModelSample."""
        idx, q, T, R, E = self._branch_model_shape(index, q_params)
        eps_in = None if epsilon is None else _np(epsilon, np.float64).reshape(T, E)
        bl, eps, lq, lp = np.empty((T, E + 1)), np.empty((T, E)), np.empty(T), np.empty(T)
        self._check(self._lib.mi_engine_branch_model_sample(
            self._h, T, (E + 3) // 2, R, _ptr(idx), q.shape[0], _ptr(q), int(seed) & (2 ** 64 - 1), int(first_sample),
            float(prior_rate), _ptr(eps_in), _ptr(bl), _ptr(eps), _ptr(lq), _ptr(lp)))
        return BranchModelSample(bl, eps, lq, lp)

    def branch_model_gradient(self, index, q_params, sample, branch_gradient, log_likelihoods, log_q_topology=None,
                              tree_weights=None, beta=1.0, prior_rate=10.0):
        """The gradient [V][2] of sum_t w_t (log p_t - log q_t) with respect to q_params for a
        BranchModelSample of the same index and q_params, from the likelihood call's
        branch_gradient [T][2n-1] and log_likelihoods [T], and log_f [T] for
        sbn_topology_gradient (mi_engine_branch_model_gradient).  Returns (gradient, log_f)."""
        idx, q, T, R, E = self._branch_model_shape(index, q_params)
        bl, eps = _np(sample.branch_lengths, np.float64).reshape(T, E + 1), _np(sample.epsilon, np.float64).reshape(T, E)
        lqb, lp = _np(sample.log_q, np.float64).reshape(T), _np(sample.log_prior, np.float64).reshape(T)
        g, ll = _np(branch_gradient, np.float64).reshape(T, E + 2), _np(log_likelihoods, np.float64).reshape(T)
        lqt = None if log_q_topology is None else _np(log_q_topology, np.float64).reshape(T)
        tw = None if tree_weights is None else _np(tree_weights, np.float64).reshape(T)
        grad, log_f = np.empty((q.shape[0], 2)), np.empty(T)
        self._check(self._lib.mi_engine_branch_model_gradient(
            self._h, T, (E + 3) // 2, R, _ptr(idx), q.shape[0], _ptr(q), _ptr(bl), _ptr(eps), _ptr(lqb), _ptr(lp),
            _ptr(g), _ptr(ll), _ptr(lqt), _ptr(tw), float(beta), float(prior_rate), _ptr(grad), _ptr(log_f)))
        return grad, log_f

    def rf_distances(self, split_index, branch_lengths=None):
        """Robinson-Foulds distances [T][T] between the trees of a split index [T][2n-1]
        (mi_engine_rf_distances); with branch_lengths [T][2n-2] also the squared
        Kuhner-Felsenstein branch scores [T][T]: returns rf, or (rf, branch_score)."""
        idx = _np(split_index, np.int32)
        if idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] < 5 or idx.shape[1] % 2 == 0:
            raise RuntimeError(f"rf_distances takes a split index [T][2n-1], n >= 3; got {idx.shape}")
        T, n = idx.shape[0], (idx.shape[1] + 1) // 2
        bl = None if branch_lengths is None else _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        rf = np.empty((T, T), np.int32)
        bs = None if bl is None else np.empty((T, T))
        self._check(self._lib.mi_engine_rf_distances(self._h, T, n, _ptr(idx), _ptr(bl), _ptr(rf), _ptr(bs)))
        return rf if bs is None else (rf, bs)

    def split_support(self, tree, trees, tree_weights=None):
        """Support of every edge of `tree` [2n-3] among `trees` [T][2n-3]: the (weighted)
        share of them that hold the edge's split, [2n-3].  `tree` is placed first in one
        split_index call, so that its edge v has index v, and its own occurrence is taken off."""
        one = _np(tree, np.int32).reshape(1, -1)
        rest = _np(trees, np.int32).reshape(-1, one.shape[1])
        E = one.shape[1]
        if tree_weights is None:
            table = self.split_index(np.concatenate([one, rest]))
            return (table.trees[:E] - 1) / rest.shape[0]
        w = _np(tree_weights, np.float64).reshape(rest.shape[0])
        # (weight 0 for the tree itself: its splits come first and add nothing)
        table = self.split_index(np.concatenate([one, rest]), tree_weights=np.concatenate([[0.0], w]))
        return table.stats[:E, 0] / w.sum()

    def pattern_mixture(self, pattern_log_likelihoods, pattern_weights, tree_log_weights=None):
        """Marginal of a mixture of trees (mi_engine_pattern_mixture): s [T][P], pattern weights
        [P], log tree weights [T] (None: log(1/T) each) -> (logsumexp_t(s[t][p] + lw_t) [P], its
        weighted sum over the patterns).  Any engine serves."""
        s = _np(pattern_log_likelihoods, np.float64)
        if s.ndim != 2:
            raise RuntimeError("pattern_mixture: pattern log-likelihoods must be [T][P]")
        T, P = s.shape
        pw = _np(pattern_weights, np.float64).reshape(P)
        lw = None if tree_log_weights is None else _np(tree_log_weights, np.float64).reshape(T)
        out, total = np.empty(P), np.empty(1)
        self._check(self._lib.mi_engine_pattern_mixture(self._h, T, P, _ptr(s), _ptr(lw), _ptr(pw),
                                                        _ptr(out), _ptr(total)))
        return out, float(total[0])

    def optimize_branch_lengths(self, parent_ids, start_branch_lengths, params=None,
                                rescaling=False, max_iterations=100, check_interval=4,
                                pack_active=True, tolerance=1e-6, min_length=1e-8,
                                max_length=10.0):
        """Maximum-likelihood branch lengths of unrooted trees within [min_length, max_length]
        (mi_engine_optimize_branch_lengths_unrooted; an extension, 4-state engines): iterated
        on the device from the Hessian call's g, H and S.  Returns a BranchOptResult."""
        n, N = self.taxon_count, self.node_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        opts = _branch_opt_options(max_iterations, check_interval, pack_active, tolerance,
                                   min_length, max_length)
        if T == 0:
            return BranchOptResult(np.empty((0, 2 * n - 2)), np.empty(0), np.empty((0, N)),
                                   np.empty((0, N)), np.empty(0, np.int32), np.empty(0, np.int32))
        bl = _np(start_branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        out = BranchOptResult(np.empty((T, 2 * n - 2)), np.empty(T), np.empty((T, N)),
                              np.empty((T, N)), np.empty(T, np.int32), np.empty(T, np.int32))
        self._check(self._lib.mi_engine_optimize_branch_lengths_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), C.addressof(opts),
            _ptr(out.branch_lengths), _ptr(out.log_likelihood), _ptr(out.gradient),
            _ptr(out.hessian), _ptr(out.iterations), _ptr(out.status)))
        return out

    def nni_apply(self, parent_ids, branch_lengths, moves):
        """Take one NNI move per tree on the device (mi_engine_nni_apply_unrooted): moves [T] are
        codes 2 v + i as nni_scan's best move gives them, or -1 for a copy.  Returns (parent ids
        [T][2n-3], branch lengths [T][2n-2]): per tree what nni_neighbour returns, bit for bit."""
        n = self.taxon_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        if T == 0:
            return np.empty((0, 2 * n - 3), np.int32), np.empty((0, 2 * n - 2))
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        mv = _np(moves, np.int32).reshape(T)
        out_pid, out_bl = np.empty((T, 2 * n - 3), np.int32), np.empty((T, 2 * n - 2))
        self._check(self._lib.mi_engine_nni_apply_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(mv), _ptr(out_pid), _ptr(out_bl)))
        return out_pid, out_bl

    def nni_search(self, parent_ids, start_branch_lengths, params=None, rescaling=False,
                   max_moves=100, pack_active=True, min_gain=1e-3, branch_opt=None):
        """NNI hill climbing per tree on the device (mi_engine_nni_search_unrooted; an extension,
        4-state engines): optimise the branch lengths, scan the neighbourhood, take the best move
        while its delta exceeds min_gain, at most max_moves times.  branch_opt: a dict of
        optimize_branch_lengths' keyword options for every round.  Returns an NniSearchResult."""
        return self._search(self._lib.mi_engine_nni_search_unrooted,
                            _nni_search_options(max_moves, pack_active, min_gain, branch_opt),
                            NniSearchResult, 1, parent_ids, start_branch_lengths, params, rescaling)

    def _search(self, fn, opts, result, width, parent_ids, start_branch_lengths, params, rescaling):
        """The host-pointer search of either kind of move: the C function, its options object,
        the result class and the words of a move in the log."""
        n = self.taxon_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        M = max(opts.max_moves, 0)
        out = result(np.empty((T, 2 * n - 3), np.int32), np.empty((T, 2 * n - 2)),
                     np.empty(T), np.empty(T), np.empty(T, np.int32),
                     np.empty((T, M) if width == 1 else (T, M, width), np.int32),
                     np.empty((T, M)), np.empty(T, np.int32), np.empty(T, np.int32))
        if T == 0:
            return out
        bl = _np(start_branch_lengths, np.float64).reshape(T, 2 * n - 2)
        pr = self._params(params, T)
        self._check(fn(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), int(rescaling), C.addressof(opts),
            _ptr(out.parent_ids), _ptr(out.branch_lengths), _ptr(out.log_likelihood),
            _ptr(out.best_delta), _ptr(out.move_count), _ptr(out.move_log), _ptr(out.move_gain),
            _ptr(out.status), _ptr(out.branch_opt_status)))
        return out

    def spr_apply(self, parent_ids, branch_lengths, moves):
        """Take one SPR move per tree on the device (mi_engine_spr_apply_unrooted): moves [T][3]
        are triples (s, dir, f) as spr_scan's best_move gives them, or (-1, -1, -1) for a copy.
        Returns (parent ids [T][2n-3], branch lengths [T][2n-2]): per tree what spr_neighbour
        returns, bit for bit."""
        n = self.taxon_count
        pid = _np(parent_ids, np.int32).reshape(-1, 2 * n - 3)
        T = pid.shape[0]
        if T == 0:
            return np.empty((0, 2 * n - 3), np.int32), np.empty((0, 2 * n - 2))
        bl = _np(branch_lengths, np.float64).reshape(T, 2 * n - 2)
        mv = _np(moves, np.int32).reshape(T, 3)
        out_pid, out_bl = np.empty((T, 2 * n - 3), np.int32), np.empty((T, 2 * n - 2))
        self._check(self._lib.mi_engine_spr_apply_unrooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(mv), _ptr(out_pid), _ptr(out_bl)))
        return out_pid, out_bl

    def spr_search(self, parent_ids, start_branch_lengths, params=None, rescaling=False,
                   max_moves=100, pack_active=True, min_gain=1e-3, radius=0, branch_opt=None):
        """SPR hill climbing per tree on the device (mi_engine_spr_search_unrooted; an extension,
        4-state engines): optimise the branch lengths, scan the SPR neighbourhood within `radius`
        (0: every move), take the best move while its delta exceeds min_gain, at most max_moves
        times.  branch_opt: a dict of optimize_branch_lengths' keyword options for every round.
        Returns an SprSearchResult."""
        return self._search(self._lib.mi_engine_spr_search_unrooted,
                            _spr_search_options(max_moves, pack_active, min_gain, radius, branch_opt),
                            SprSearchResult, 3, parent_ids, start_branch_lengths, params, rescaling)

    def _phylo_gradients(self, ll, blocks, site, subst):
        """Per-tree PhyloGradient objects over row views of the freshly allocated result
        arrays of one call (no per-tree copies: 1000 trees cost ~0.3 ms instead of ~1.1)."""
        if self.category_count > 1 and site is not None:
            blocks = dict(blocks, site_model=site.reshape(-1, 1))
        if self.is_gtr and subst is not None:
            blocks = dict(blocks, substitution_model=subst)
        names = list(blocks)
        rows = [list(blocks[k]) for k in names]  # lists of row views
        lls = ll.tolist()
        if len(names) == 1:
            (a,), (ra,) = names, rows
            return [PhyloGradient(l, {a: x}) for l, x in zip(lls, ra)]
        if len(names) == 2:
            (a, b), (ra, rb) = names, rows
            return [PhyloGradient(l, {a: x, b: y}) for l, x, y in zip(lls, ra, rb)]
        return [PhyloGradient(l, dict(zip(names, r))) for l, *r in zip(lls, *rows)]

    def rooted_log_likelihoods(self, parent_ids, branch_lengths, params=None, rates=None,
                               node_heights=None, node_bounds=None, rescaling=False,
                               with_jacobian=True):
        """Engine::LogLikelihoods(const RootedTreeCollection&) (with_jacobian=True) or
        Engine::UnrootedLogLikelihoods(const RootedTreeCollection&) (False)."""
        n, N = self.taxon_count, self.node_count
        pid = _np(parent_ids, np.int32).reshape(-1, N - 1)
        T = pid.shape[0]
        if T == 0:
            return np.empty(0)
        bl = _np(branch_lengths, np.float64).reshape(T, N)
        pr = self._params(params, T)
        r = None if rates is None else _np(rates, np.float64).reshape(T, N - 1)
        h = None if node_heights is None else _np(node_heights, np.float64).reshape(T, N)
        b = None if node_bounds is None else _np(node_bounds, np.float64).reshape(T, N)
        out = np.empty(T)
        self._check(self._lib.mi_engine_log_likelihoods_rooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), _ptr(r), _ptr(h), _ptr(b),
            int(with_jacobian), int(rescaling), _ptr(out)))
        return out

    def rooted_gradients(self, parent_ids, branch_lengths, params, rates, rate_counts,
                         node_heights, node_bounds, height_ratios, rescaling=False):
        """Engine::Gradients(const RootedTreeCollection&, ...) -> [PhyloGradient]."""
        n, N = self.taxon_count, self.node_count
        pid = _np(parent_ids, np.int32).reshape(-1, N - 1)
        T = pid.shape[0]
        if T == 0:
            return []
        bl = _np(branch_lengths, np.float64).reshape(T, N)
        pr = self._params(params, T)
        r = _np(rates, np.float64).reshape(T, N - 1)
        rc = _np(rate_counts, np.int32).reshape(T)
        h = _np(node_heights, np.float64).reshape(T, N)
        b = _np(node_bounds, np.float64).reshape(T, N)
        ra = _np(height_ratios, np.float64).reshape(T, n - 1)
        ll, gr, gc = np.empty(T), np.empty((T, n - 1)), np.empty((T, N - 1))
        site, subst = np.empty(T), np.empty((T, 8))
        self._check(self._lib.mi_engine_gradients_rooted(
            self._h, T, _ptr(pid), _ptr(bl), _ptr(pr), _ptr(r), _ptr(rc), _ptr(h), _ptr(b),
            _ptr(ra), int(rescaling), _ptr(ll), _ptr(gr), _ptr(gc), _ptr(site), _ptr(subst)))
        out = []
        for t in range(T):
            gm = {"ratios_root_height": gr[t].copy(),
                  "clock_model": gc[t, :1].copy() if rc[t] == 1 else gc[t].copy()}
            if self.category_count > 1:
                gm["site_model"] = site[t:t + 1].copy()
            if self.is_gtr:
                gm["substitution_model"] = subst[t].copy()
            out.append(PhyloGradient(float(ll[t]), gm))
        return out

    # ---- device-pointer path (raw pointers, e.g. torch tensors' data_ptr()) ------
    def reserve(self, tree_count, for_gradients):
        self._check(self._lib.mi_engine_reserve(self._h, tree_count, int(for_gradients)))

    def log_likelihoods_device(self, stream, T, parent_ids, branch_lengths, params, out_ll,
                               rescaling=False):
        self._check(self._lib.mi_engine_log_likelihoods_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, params, int(rescaling), out_ll))

    def gradients_device(self, stream, T, parent_ids, branch_lengths, params, out_ll,
                         out_branch, out_site=None, out_subst=None, rescaling=False):
        self._check(self._lib.mi_engine_gradients_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, params, int(rescaling), out_ll,
            out_branch, out_site, out_subst))

    def branch_hessian_device(self, stream, T, parent_ids, branch_lengths, params, out_hess,
                              out_ll=None, out_branch=None, out_gsq=None, rescaling=False):
        """mi_engine_branch_hessian_unrooted_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_branch_hessian_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, params, int(rescaling), out_ll,
            out_branch, out_hess, out_gsq))

    def reserve_hessian(self, tree_count):
        """mi_engine_reserve_hessian: workspace of a Hessian call (graph capture)."""
        self._check(self._lib.mi_engine_reserve_hessian(self._h, int(tree_count)))

    def nni_scan_device(self, stream, T, parent_ids, branch_lengths, params, out_delta,
                        out_ll=None, out_best=None, rescaling=False):
        """mi_engine_nni_scan_unrooted_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_nni_scan_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, params, int(rescaling), out_ll,
            out_delta, out_best))

    def spr_scan_device(self, stream, T, parent_ids, branch_lengths, params, out_best_target, out_best_delta,
                        out_ll=None, out_best_move=None, out_delta=None, rescaling=False, radius=0):
        """mi_engine_spr_scan_unrooted_device: device pointers, enqueued on `stream` (no allocation
        after reserve_spr_scan)."""
        self._check(self._lib.mi_engine_spr_scan_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, params, int(rescaling), int(radius), out_ll,
            out_best_target, out_best_delta, out_best_move, out_delta))

    def reserve_spr_scan(self, tree_count):
        """mi_engine_reserve_spr_scan: workspace of an SPR scan (graph capture)."""
        self._check(self._lib.mi_engine_reserve_spr_scan(self._h, int(tree_count)))

    def reserve_nni_scan(self, tree_count):
        """mi_engine_reserve_nni_scan: workspace of an NNI scan (graph capture)."""
        self._check(self._lib.mi_engine_reserve_nni_scan(self._h, int(tree_count)))

    def ancestral_states_device(self, stream, T, parent_ids, branch_lengths, params,
                                out_state_posteriors, out_ll=None, out_map_states=None,
                                out_category_posteriors=None, out_pattern_rates=None,
                                out_tip_posteriors=None, rescaling=False):
        """mi_engine_ancestral_states_unrooted_device: device pointers, enqueued on `stream` (no
        allocation after reserve_ancestral(T))."""
        self._check(self._lib.mi_engine_ancestral_states_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, params, int(rescaling), out_ll,
            out_state_posteriors, out_map_states, out_category_posteriors, out_pattern_rates,
            out_tip_posteriors))

    def reserve_ancestral(self, tree_count):
        """mi_engine_reserve_ancestral: workspace of an ancestral-state call (graph capture)."""
        self._check(self._lib.mi_engine_reserve_ancestral(self._h, int(tree_count)))

    def placement_device(self, stream, T, parent_ids, branch_lengths, params, Q, C, query_states,
                         column_pattern, column_weights, G, pendant_lengths, out_edge_ll, out_ll=None,
                         out_pendant_index=None, out_best_edge=None, out_lwr=None, out_tables=None,
                         rescaling=False):
        """mi_engine_placement_unrooted_device: device pointers (the pendant lengths too), enqueued
        on `stream` (no allocation after reserve_placement)."""
        self._check(self._lib.mi_engine_placement_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, params, int(rescaling), Q, C, query_states,
            column_pattern, column_weights, G, pendant_lengths, out_ll, out_edge_ll, out_pendant_index,
            out_best_edge, out_lwr, out_tables))

    def reserve_placement(self, tree_count, query_count, column_count, pendant_count):
        """mi_engine_reserve_placement: workspace of a placement call (graph capture)."""
        self._check(self._lib.mi_engine_reserve_placement(self._h, int(tree_count), int(query_count),
                                                          int(column_count), int(pendant_count)))

    def optimize_branch_lengths_device(self, stream, T, parent_ids, start_branch_lengths, params,
                                       out_branch_lengths, out_ll, out_status, out_branch=None,
                                       out_hess=None, out_iterations=None, rescaling=False,
                                       max_iterations=100, check_interval=4, pack_active=True,
                                       tolerance=1e-6, min_length=1e-8, max_length=10.0):
        """mi_engine_optimize_branch_lengths_unrooted_device: device pointers.  The call
        synchronises `stream` at its check points, so it cannot be captured in a graph."""
        opts = _branch_opt_options(max_iterations, check_interval, pack_active, tolerance,
                                   min_length, max_length)
        self._check(self._lib.mi_engine_optimize_branch_lengths_unrooted_device(
            self._h, stream, T, parent_ids, start_branch_lengths, params, int(rescaling),
            C.addressof(opts), out_branch_lengths, out_ll, out_branch, out_hess, out_iterations,
            out_status))

    def reserve_branch_opt(self, tree_count):
        """mi_engine_reserve_branch_opt: workspace of an optimisation call of that size."""
        self._check(self._lib.mi_engine_reserve_branch_opt(self._h, int(tree_count)))

    def nni_apply_device(self, stream, T, parent_ids, branch_lengths, moves, out_parent_ids,
                         out_branch_lengths):
        """mi_engine_nni_apply_unrooted_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_nni_apply_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, moves, out_parent_ids,
            out_branch_lengths))

    def nni_search_device(self, stream, T, parent_ids, start_branch_lengths, params,
                          out_parent_ids, out_branch_lengths, out_ll, out_move_count, out_status,
                          out_best_delta=None, out_move_log=None, out_move_gain=None,
                          out_branch_opt_status=None, rescaling=False, max_moves=100,
                          pack_active=True, min_gain=1e-3, branch_opt=None):
        """mi_engine_nni_search_unrooted_device: device pointers.  The call synchronises `stream`
        every round, so it cannot be captured in a graph."""
        opts = _nni_search_options(max_moves, pack_active, min_gain, branch_opt)
        self._check(self._lib.mi_engine_nni_search_unrooted_device(
            self._h, stream, T, parent_ids, start_branch_lengths, params, int(rescaling),
            C.addressof(opts), out_parent_ids, out_branch_lengths, out_ll, out_best_delta,
            out_move_count, out_move_log, out_move_gain, out_status, out_branch_opt_status))

    def reserve_nni_search(self, tree_count):
        """mi_engine_reserve_nni_search: workspace of a search or apply call of that size."""
        self._check(self._lib.mi_engine_reserve_nni_search(self._h, int(tree_count)))

    def spr_apply_device(self, stream, T, parent_ids, branch_lengths, moves, out_parent_ids,
                         out_branch_lengths):
        """mi_engine_spr_apply_unrooted_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_spr_apply_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, moves, out_parent_ids,
            out_branch_lengths))

    def spr_search_device(self, stream, T, parent_ids, start_branch_lengths, params,
                          out_parent_ids, out_branch_lengths, out_ll, out_move_count, out_status,
                          out_best_delta=None, out_move_log=None, out_move_gain=None,
                          out_branch_opt_status=None, rescaling=False, max_moves=100,
                          pack_active=True, min_gain=1e-3, radius=0, branch_opt=None):
        """mi_engine_spr_search_unrooted_device: device pointers.  The call synchronises `stream`
        every round, so it cannot be captured in a graph."""
        opts = _spr_search_options(max_moves, pack_active, min_gain, radius, branch_opt)
        self._check(self._lib.mi_engine_spr_search_unrooted_device(
            self._h, stream, T, parent_ids, start_branch_lengths, params, int(rescaling),
            C.addressof(opts), out_parent_ids, out_branch_lengths, out_ll, out_best_delta,
            out_move_count, out_move_log, out_move_gain, out_status, out_branch_opt_status))

    def reserve_spr_search(self, tree_count):
        """mi_engine_reserve_spr_search: workspace of a search or apply call of that size."""
        self._check(self._lib.mi_engine_reserve_spr_search(self._h, int(tree_count)))

    def pattern_log_likelihoods_device(self, stream, T, parent_ids, branch_lengths, params,
                                       out_pattern_ll, out_ll=None, rescaling=False):
        """mi_engine_pattern_log_likelihoods_unrooted_device: device pointers, enqueued on
        `stream` (no allocation after reserve(T, False))."""
        self._check(self._lib.mi_engine_pattern_log_likelihoods_unrooted_device(
            self._h, stream, T, parent_ids, branch_lengths, params, int(rescaling), out_ll,
            out_pattern_ll))

    def rell_device(self, stream, B, T, P, pattern_ll, replicate_weights, out_bp, out_replicate_ll=None,
                    out_best=None, out_elw=None):
        """mi_engine_rell_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_rell_device(
            self._h, stream, int(B), int(T), int(P), pattern_ll, replicate_weights, out_replicate_ll,
            out_best, out_bp, out_elw))

    def reserve_rell(self, replicate_count, tree_count, pattern_count):
        """mi_engine_reserve_rell: workspace of a RELL call of that size."""
        self._check(self._lib.mi_engine_reserve_rell(self._h, int(replicate_count), int(tree_count),
                                                     int(pattern_count)))

    def bootstrap_weights_device(self, stream, P, weights, B, sites, seed, first_replicate, out_weights):
        """mi_engine_bootstrap_weights_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_bootstrap_weights_device(
            self._h, stream, int(P), weights, int(B), int(sites), int(seed), int(first_replicate), out_weights))

    def reserve_bootstrap_weights(self, replicate_count, pattern_count):
        """mi_engine_reserve_bootstrap_weights: workspace of a sampler call of that size."""
        self._check(self._lib.mi_engine_reserve_bootstrap_weights(self._h, int(replicate_count), int(pattern_count)))

    def topology_tests_device(self, stream, T, P, pattern_ll, weights, sites, replicates, seed, first_replicate,
                              out_table, out_counts, out_mean=None, out_replicate_ll=None, out_best=None):
        """mi_engine_topology_tests_device: device pointers but sites and replicates (host
        sequences), enqueued on `stream`."""
        si, reps = _np(sites, np.int64).reshape(-1), _np(replicates, np.int32).reshape(-1)
        if si.size != reps.size:
            raise RuntimeError("topology tests: sites and replicates must have one entry per block")
        self._check(self._lib.mi_engine_topology_tests_device(
            self._h, stream, int(T), int(P), pattern_ll, weights, si.size, _ptr(si), _ptr(reps), int(seed),
            int(first_replicate), out_table, out_counts, out_mean, out_replicate_ll, out_best))

    def reserve_topology_tests(self, tree_count, pattern_count, max_replicate_count):
        """mi_engine_reserve_topology_tests: workspace of the tests for that many trees, patterns
        and replicates of the largest block (the *_device form then allocates nothing)."""
        self._check(self._lib.mi_engine_reserve_topology_tests(self._h, int(tree_count), int(pattern_count),
                                                               int(max_replicate_count)))

    def pairwise_distances_device(self, stream, B, replicate_weights, params, out_distances,
                                  out_pair_counts=None, out_pair_status=None, min_length=1e-8,
                                  max_length=10.0, tolerance=1e-10, max_iterations=50):
        """mi_engine_pairwise_distances_device: device pointers, enqueued on `stream`."""
        opts = _distance_options(min_length, max_length, tolerance, max_iterations)
        self._check(self._lib.mi_engine_pairwise_distances_device(
            self._h, stream, int(B), replicate_weights, params, C.addressof(opts), out_distances,
            out_pair_counts, out_pair_status))

    def neighbour_joining_device(self, stream, B, n, distances, out_parent_ids, out_branch_lengths,
                                 min_length=1e-8, max_length=10.0):
        """mi_engine_neighbour_joining_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_neighbour_joining_device(
            self._h, stream, int(B), int(n), distances, float(min_length), float(max_length),
            out_parent_ids, out_branch_lengths))

    def starting_trees_device(self, stream, B, replicate_weights, params, out_parent_ids,
                              out_branch_lengths, out_distances=None, min_length=1e-8,
                              max_length=10.0, tolerance=1e-10, max_iterations=50):
        """mi_engine_starting_trees_unrooted_device: device pointers, enqueued on `stream`."""
        opts = _distance_options(min_length, max_length, tolerance, max_iterations)
        self._check(self._lib.mi_engine_starting_trees_unrooted_device(
            self._h, stream, int(B), replicate_weights, params, C.addressof(opts), out_parent_ids,
            out_branch_lengths, out_distances))

    def reserve_start_trees(self, replicate_count):
        """mi_engine_reserve_start_trees: workspace of the three calls above for that many
        replicates (their *_device forms then allocate nothing: graph capture)."""
        self._check(self._lib.mi_engine_reserve_start_trees(self._h, int(replicate_count)))

    def split_index_device(self, stream, T, n, parent_ids, split_capacity, out_split_index, out_split_count,
                           out_split_bits, out_split_first, out_split_trees, out_split_stats=None,
                           branch_lengths=None, tree_weights=None):
        """mi_engine_split_index_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_split_index_device(
            self._h, stream, int(T), int(n), parent_ids, branch_lengths, tree_weights, int(split_capacity),
            out_split_index, out_split_count, out_split_bits, out_split_first, out_split_trees,
            out_split_stats))

    def rf_distances_device(self, stream, T, n, split_index, out_rf, out_branch_score=None,
                            branch_lengths=None):
        """mi_engine_rf_distances_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_rf_distances_device(
            self._h, stream, int(T), int(n), split_index, branch_lengths, out_rf, out_branch_score))

    def reserve_splits(self, tree_count, taxon_count):
        """mi_engine_reserve_splits: workspace of the two calls above for that many trees of
        that taxon count (their *_device forms then allocate nothing: graph capture)."""
        self._check(self._lib.mi_engine_reserve_splits(self._h, int(tree_count), int(taxon_count)))

    def sbn_index_device(self, stream, T, n, parent_ids, support_tree_count, rootsplit_capacity, pcsp_capacity,
                         out_root_index, out_slot_index, out_counts, out_split_bits, out_pcsp_clades,
                         out_parent_range, out_pcsp_parent):
        """mi_engine_sbn_index_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_sbn_index_device(
            self._h, stream, int(T), int(n), parent_ids, int(support_tree_count), int(rootsplit_capacity),
            int(pcsp_capacity), out_root_index, out_slot_index, out_counts, out_split_bits, out_pcsp_clades,
            out_parent_range, out_pcsp_parent))

    def sbn_log_prob_device(self, stream, T, n, parent_ids, root_index, slot_index, rootsplit_count, pcsp_count,
                            parent_count, parent_range, log_params, normalized, out_rooting_log_prob, out_log_q,
                            out_log_expected_counts=None, tree_weights=None):
        """mi_engine_sbn_log_prob_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_sbn_log_prob_device(
            self._h, stream, int(T), int(n), parent_ids, root_index, slot_index, int(rootsplit_count),
            int(pcsp_count), int(parent_count), parent_range, log_params, int(bool(normalized)), tree_weights,
            out_rooting_log_prob, out_log_q, out_log_expected_counts))

    def sbn_normalize_device(self, stream, rootsplit_count, pcsp_count, parent_count, parent_range, log_params,
                             out_log_params):
        """mi_engine_sbn_normalize_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_sbn_normalize_device(
            self._h, stream, int(rootsplit_count), int(pcsp_count), int(parent_count), parent_range, log_params,
            out_log_params))

    def sbn_train_device(self, stream, T, n, parent_ids, root_index, slot_index, rootsplit_count, pcsp_count,
                         parent_count, parent_range, method, alpha, max_iter, score_epsilon, out_log_params,
                         out_score_history, out_iterations, tree_weights=None):
        """mi_engine_sbn_train_device: device pointers; synchronises `stream` (one double is read
        per EM iteration), so it cannot be captured in a graph."""
        self._check(self._lib.mi_engine_sbn_train_device(
            self._h, stream, int(T), int(n), parent_ids, root_index, slot_index, int(rootsplit_count),
            int(pcsp_count), int(parent_count), parent_range, tree_weights, 0 if method == "sa" else 1,
            float(alpha), int(max_iter), float(score_epsilon), out_log_params, out_score_history, out_iterations))

    def sbn_descent_device(self, stream, support_tree_count, n, parent_ids, root_index, slot_index,
                           rootsplit_count, pcsp_count, pcsp_parent, out_descent):
        """mi_engine_sbn_descent_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_sbn_descent_device(
            self._h, stream, int(support_tree_count), int(n), parent_ids, root_index, slot_index,
            int(rootsplit_count), int(pcsp_count), pcsp_parent, out_descent))

    def sbn_sample_device(self, stream, K, n, rootsplit_count, pcsp_count, parent_count, parent_range, descent,
                          log_params, seed, first_sample, out_parent_ids, out_root_edge, out_sampled_params,
                          out_log_prob, out_cdf=None):
        """mi_engine_sbn_sample_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_sbn_sample_device(
            self._h, stream, int(K), int(n), int(rootsplit_count), int(pcsp_count), int(parent_count),
            parent_range, descent, log_params, int(seed) & (2 ** 64 - 1), int(first_sample), out_parent_ids,
            out_root_edge, out_sampled_params, out_log_prob, out_cdf))

    def sbn_topology_gradient_device(self, stream, T, n, parent_ids, root_index, slot_index, rootsplit_count,
                                     pcsp_count, parent_count, parent_range, log_params, normalized, log_f,
                                     estimator, out_gradient, out_factors, out_log_q):
        """mi_engine_sbn_topology_gradient_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_sbn_topology_gradient_device(
            self._h, stream, int(T), int(n), parent_ids, root_index, slot_index, int(rootsplit_count),
            int(pcsp_count), int(parent_count), parent_range, log_params, int(bool(normalized)), log_f,
            _sbn_factors(estimator), out_gradient, out_factors, out_log_q))

    def reserve_sbn(self, tree_count, taxon_count):
        """mi_engine_reserve_sbn: workspace of the SBN calls for that many trees of that taxon
        count (sbn_log_prob_device and sbn_normalize_device then allocate nothing: graph capture)."""
        self._check(self._lib.mi_engine_reserve_sbn(self._h, int(tree_count), int(taxon_count)))

    def psp_table_device(self, stream, rootsplit_count, pcsp_count, pcsp_clades, out_psp_of_pcsp, out_counts):
        """mi_engine_psp_table_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_psp_table_device(
            self._h, stream, int(rootsplit_count), int(pcsp_count), pcsp_clades, out_psp_of_pcsp, out_counts))

    def psp_index_device(self, stream, T, n, root_index, slot_index, rootsplit_count, pcsp_count, psp_of_pcsp,
                         variable_count, rows, out_index):
        """mi_engine_psp_index_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_psp_index_device(
            self._h, stream, int(T), int(n), root_index, slot_index, int(rootsplit_count), int(pcsp_count),
            psp_of_pcsp, int(variable_count), int(rows), out_index))

    def branch_model_sample_device(self, stream, T, n, rows, index, variable_count, q_params, seed, first_sample,
                                   prior_rate, out_branch_lengths, out_epsilon, out_log_q, out_log_prior,
                                   epsilon_in=None):
        """mi_engine_branch_model_sample_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_branch_model_sample_device(
            self._h, stream, int(T), int(n), int(rows), index, int(variable_count), q_params,
            int(seed) & (2 ** 64 - 1), int(first_sample), float(prior_rate), epsilon_in, out_branch_lengths,
            out_epsilon, out_log_q, out_log_prior))

    def branch_model_gradient_device(self, stream, T, n, rows, index, variable_count, q_params, branch_lengths,
                                     epsilon, log_q_branch, log_prior, branch_gradient, log_likelihoods, beta,
                                     prior_rate, out_gradient, out_log_f, log_q_topology=None, tree_weights=None):
        """mi_engine_branch_model_gradient_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_branch_model_gradient_device(
            self._h, stream, int(T), int(n), int(rows), index, int(variable_count), q_params, branch_lengths,
            epsilon, log_q_branch, log_prior, branch_gradient, log_likelihoods, log_q_topology, tree_weights,
            float(beta), float(prior_rate), out_gradient, out_log_f))

    def reserve_branch_model(self, tree_count, taxon_count, rows=3):
        """mi_engine_reserve_branch_model: workspace of branch_model_gradient_device for that many
        trees and rows of that taxon count (it then allocates nothing: graph capture)."""
        self._check(self._lib.mi_engine_reserve_branch_model(self._h, int(tree_count), int(taxon_count), int(rows)))

    def pattern_mixture_device(self, stream, T, P, pattern_ll, pattern_weights, out_pattern_log_marginal,
                               out_log_marginal, tree_log_weights=None):
        """mi_engine_pattern_mixture_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_engine_pattern_mixture_device(
            self._h, stream, int(T), int(P), pattern_ll, tree_log_weights, pattern_weights,
            out_pattern_log_marginal, out_log_marginal))

    def reserve_reduced(self, tree_count, index_count):
        """mi_engine_reserve_reduced: workspace of a fused-reduction call (graph capture)."""
        self._check(self._lib.mi_engine_reserve_reduced(self._h, int(tree_count), int(index_count)))

    def vi_create(self, support_parent_ids, log_params, q_params, particle_count=10, rows=3, estimator="vimco",
                  anneal_steps=0, max_steps=1000, prior_rate=10.0, step_size=(0.001, 0.001), sbn_step_size=0.001,
                  step_decay=0.99, adam_beta0=0.9, adam_beta1=0.999, adam_epsilon=1e-8, seed=0, first_sample=0,
                  model_params=None):
        """A device-resident variational fit over the support of support_parent_ids [T0][2n-3]
        (mi_engine_vi_create), from log_params [P] and q_params [V][2] (for instance
        lognormal_mode_match's); model_params: the one parameter row every particle takes.
        Returns a VariationalFit."""
        if estimator not in ("plain", "vimco"):
            raise RuntimeError(f"vi_create: estimator must be 'plain' or 'vimco', got {estimator!r}")
        pid = np.empty((0, 2 * self.taxon_count - 3), np.int32)   # (None: the two tables alone, for update())
        if support_parent_ids is not None:
            pid = _np(support_parent_ids, np.int32).reshape(-1, 2 * self.taxon_count - 3)
        phi, q = _np(log_params, np.float64).reshape(-1), _np(q_params, np.float64).reshape(-1, 2)
        mp = None if model_params is None or self.param_count == 0 else _np(model_params, np.float64).reshape(self.param_count)
        o = _capi.ViOptions()
        self._check(self._lib.mi_vi_default_options(C.byref(o)))
        o.particle_count, o.rows, o.estimator = int(particle_count), int(rows), _SBN_FACTORS[estimator]
        o.anneal_steps, o.max_steps, o.prior_rate = int(anneal_steps), int(max_steps), float(prior_rate)
        o.step_size[0], o.step_size[1] = (float(x) for x in np.broadcast_to(step_size, 2))
        o.sbn_step_size, o.step_decay = float(sbn_step_size), float(step_decay)
        o.adam_beta0, o.adam_beta1, o.adam_epsilon = float(adam_beta0), float(adam_beta1), float(adam_epsilon)
        o.seed, o.first_sample = int(seed) & (2 ** 64 - 1), int(first_sample)
        h = C.c_void_p()
        self._check(self._lib.mi_engine_vi_create(self._h, pid.shape[0], _ptr(pid) if len(pid) else None, _ptr(mp), phi.shape[0], _ptr(phi),
                                                  q.shape[0], _ptr(q), C.byref(o), C.byref(h)))
        return VariationalFit(self, h, pid, mp, o)

    def gp_create(self, parent_ids, branch_lengths=None, params=None, rescaling_threshold=None):
        """Generalized pruning over the subsplit DAG of the rooted topologies parent_ids [T][2n-2]
        (mi_engine_gp_create).  branch_lengths [T][2n-1]: a hot start (the mean
        over the trees that hold an entry), else 0.1 everywhere; params: the one model parameter
        row; rescaling_threshold None: the default 2^-256.  Returns a GeneralizedPruning."""
        pid = _np(parent_ids, np.int32)
        if pid.ndim == 1:
            pid = pid[None, :]
        if pid.ndim != 2 or pid.shape[1] < 4 or pid.shape[1] % 2:
            raise RuntimeError("gp_create: parent_ids must be [T][2n-2]")
        n = pid.shape[1] // 2 + 1
        bl = None
        if branch_lengths is not None:
            bl = _np(branch_lengths, np.float64).reshape(-1, 2 * n - 1)
            if bl.shape[0] != pid.shape[0]:
                raise RuntimeError("gp_create: branch_lengths must be [T][2n-1]")
        mp = None if params is None or self.param_count == 0 else _np(params, np.float64).reshape(self.param_count)
        h = C.c_void_p()
        self._check(self._lib.mi_engine_gp_create(self._h, pid.shape[0], n, _ptr(pid), _ptr(bl), _ptr(mp),
                                                  0.0 if rescaling_threshold is None else float(rescaling_threshold),
                                                  C.byref(h)))
        return GeneralizedPruning(self, h)

    def gp_create_dag(self, parent_ids, branch_lengths=None):
        """A DAG-only GeneralizedPruning on any engine (mi_engine_gp_create_dag): the
        DAG, numbering, initial q and b of gp_create, no vectors.  It serves the structure, b / q and
        tree calls (index, log q, training, sampling, enumeration) and refuses whatever needs vectors."""
        pid = _np(parent_ids, np.int32)
        if pid.ndim == 1:
            pid = pid[None, :]
        if pid.ndim != 2 or pid.shape[1] < 4 or pid.shape[1] % 2:
            raise RuntimeError("gp_create_dag: parent_ids must be [T][2n-2]")
        n = pid.shape[1] // 2 + 1
        bl = None
        if branch_lengths is not None:
            bl = _np(branch_lengths, np.float64).reshape(-1, 2 * n - 1)
            if bl.shape[0] != pid.shape[0]:
                raise RuntimeError("gp_create_dag: branch_lengths must be [T][2n-1]")
        h = C.c_void_p()
        self._check(self._lib.mi_engine_gp_create_dag(self._h, pid.shape[0], n, _ptr(pid), _ptr(bl), C.byref(h)))
        return GeneralizedPruning(self, h)

    def deroot_trees(self, parent_ids, branch_lengths=None):
        """Rooted trees parent_ids [T][2n-2] (root 2n-2), de-rooted as Node::Deroot does and renumbered
        in the unrooted convention (mi_engine_deroot_trees): a DerootedTrees."""
        pid = _np(parent_ids, np.int32)
        if pid.ndim == 1:
            pid = pid[None, :]
        if pid.ndim != 2 or pid.shape[1] < 4 or pid.shape[1] % 2:
            raise RuntimeError("deroot_trees: parent_ids must be [T][2n-2]")
        T, n = pid.shape[0], pid.shape[1] // 2 + 1
        bl = out_bl = None
        if branch_lengths is not None:
            bl = _np(branch_lengths, np.float64).reshape(-1, 2 * n - 1)
            if bl.shape[0] != T:
                raise RuntimeError("deroot_trees: branch_lengths must be [T][2n-1]")
            out_bl = np.empty((T, 2 * n - 2))
        out, edge = np.empty((T, 2 * n - 3), np.int32), np.empty(T, np.int32)
        self._check(self._lib.mi_engine_deroot_trees(self._h, T, n, _ptr(pid), _ptr(bl), _ptr(out), _ptr(out_bl), _ptr(edge)))
        return DerootedTrees(out, out_bl, edge)

    def deroot_trees_mapped(self, parent_ids, branch_lengths=None):
        """deroot_trees plus new_id [T][2n-1] (mi_engine_deroot_trees_mapped): the unrooted id under which
        every rooted node's edge lands (both root children: root_edge; the root: -1)."""
        pid = _np(parent_ids, np.int32)
        if pid.ndim == 1:
            pid = pid[None, :]
        if pid.ndim != 2 or pid.shape[1] < 4 or pid.shape[1] % 2:
            raise RuntimeError("deroot_trees_mapped: parent_ids must be [T][2n-2]")
        T, n = pid.shape[0], pid.shape[1] // 2 + 1
        bl = out_bl = None
        if branch_lengths is not None:
            bl = _np(branch_lengths, np.float64).reshape(-1, 2 * n - 1)
            if bl.shape[0] != T:
                raise RuntimeError("deroot_trees_mapped: branch_lengths must be [T][2n-1]")
            out_bl = np.empty((T, 2 * n - 2))
        out, edge, new_id = np.empty((T, 2 * n - 3), np.int32), np.empty(T, np.int32), np.empty((T, 2 * n - 1), np.int32)
        self._check(self._lib.mi_engine_deroot_trees_mapped(self._h, T, n, _ptr(pid), _ptr(bl), _ptr(out), _ptr(out_bl),
                                                            _ptr(edge), _ptr(new_id)))
        return DerootedTrees(out, out_bl, edge, new_id)

    def deroot_trees_mapped_device(self, stream, T, n, parent_ids, branch_lengths, out_parent_ids, out_branch_lengths,
                                   out_root_edge, out_new_id):
        """mi_engine_deroot_trees_mapped_device: device pointers, enqueued on `stream`; needs reserve_deroot."""
        self._check(self._lib.mi_engine_deroot_trees_mapped_device(self._h, stream, T, n, parent_ids, branch_lengths,
                                                                   out_parent_ids, out_branch_lengths, out_root_edge,
                                                                   out_new_id))

    def reserve_deroot(self, tree_count, taxon_count):
        self._check(self._lib.mi_engine_reserve_deroot(self._h, tree_count, taxon_count))

    def deroot_trees_device(self, stream, T, n, parent_ids, branch_lengths, out_parent_ids, out_branch_lengths,
                            out_root_edge):
        """mi_engine_deroot_trees_device: device pointers, enqueued on `stream`; needs reserve_deroot."""
        self._check(self._lib.mi_engine_deroot_trees_device(self._h, stream, T, n, parent_ids, branch_lengths,
                                                            out_parent_ids, out_branch_lengths, out_root_edge))

    def check_status(self, stream=None):
        self._check(self._lib.mi_engine_check_status(self._h, stream))

    def profile_begin(self, max_calls):
        self._check(self._lib.mi_engine_profile_begin(self._h, max_calls))

    def profile_collect(self, capacity):
        out = (C.c_double * capacity)()
        cnt = C.c_int32()
        self._check(self._lib.mi_engine_profile_collect(self._h, out, capacity, C.byref(cnt)))
        return [out[i] for i in range(cnt.value)]

    def profile_begin_phases(self, max_calls):
        self._check(self._lib.mi_engine_profile_begin_phases(self._h, max_calls))

    def profile_collect_phases(self, capacity):
        """(total ms per call, [set-up, post-order, pre-order / main walk, rest] ms per call,
        evaluations in the first walk launch) -- include/mi_phylo.h"""
        out = (C.c_double * capacity)()
        ph = (C.c_double * (4 * capacity))()
        cnt, first = C.c_int32(), C.c_int32()
        self._check(self._lib.mi_engine_profile_collect_phases(
            self._h, out, ph, capacity, C.byref(cnt), C.byref(first)))
        return ([out[i] for i in range(cnt.value)],
                [[ph[4 * i + k] for k in range(4)] for i in range(cnt.value)], first.value)

    def shard_devices(self):
        """HIP device ordinal of every shard (a single-device engine: its one device)."""
        k = self._lib.mi_engine_shard_count(self._h)
        return [self._lib.mi_engine_shard_device(self._h, i) for i in range(k)]

    def last_call_info(self):
        name, ev, gev = C.c_char_p(), C.c_int64(), C.c_int64()
        self._check(self._lib.mi_engine_last_call_info(self._h, C.byref(name), C.byref(ev),
                                                       C.byref(gev)))
        return name.value.decode(), ev.value, gev.value

    def last_call_path(self):
        """mi_engine_last_call_path: one line saying which kernels / stores the last call used."""
        return self._lib.mi_engine_last_call_path(self._h).decode()

    def last_call_launches(self):
        """(walk-kernel launches of the last call, arena-budget back-offs since creation)"""
        a, b = C.c_int32(), C.c_int32()
        self._check(self._lib.mi_engine_last_call_launches(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


@dataclass
class ViState:
    """VariationalFit.state: the whole state of a fit (include/mi_phylo.h, mi_vi_get_state)."""
    log_params: np.ndarray    # [P] the SBN's unnormalised log parameters
    q_params: np.ndarray      # [V][2] mu, sigma
    sbn_moments: np.ndarray   # [2][P] Adam's m, then v
    q_moments: np.ndarray     # [2][V][2]
    b0: float                 # adam_beta0 ** successes, by repeated rounded multiplication
    b1: float
    step_size: np.ndarray     # [2] the mu and the sigma column's
    sbn_step_size: float
    steps: int                # t: steps so far, failed ones included
    successes: int            # a
    first_sample: int         # the sample base: step t draws first_sample + t K + k


TRACE_COLUMNS = ("beta", "elbo", "bound", "step_size_mu", "step_size_sigma", "success")


class VariationalFit:
    """A device-resident variational fit (mi_vi, include/mi_phylo.h), made by
    Engine.vi_create.  The engine must outlive it."""

    def __init__(self, engine, handle, support_ids, model_params, options):
        self.engine, self._h, self._lib = engine, handle, engine._lib
        self.support_ids, self.model_params, self.options = support_ids, model_params, options
        sizes = np.zeros(9, np.int32)
        self._check(self._lib.mi_vi_sizes(self._h, sizes.ctypes.data_as(_capi.I32P)))
        (self.taxon_count, self.particle_count, self.rows, self.rootsplit_count, self.pcsp_count,
         self.parent_count, self.variable_count, self.max_steps, self.parameter_count) = (int(x) for x in sizes)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(_capi.last_error())

    def close(self):
        if self._h is not None:
            if self.engine._h is not None:   # (a fit whose engine is gone already cannot be synchronised: left alone)
                self._lib.mi_vi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step_device(self, stream=None):
        """Enqueue one step on `stream` (mi_vi_step_device): nothing is read back, so a caller may
        capture it in a graph on one stream; every replay is the next step."""
        self._check(self._lib.mi_vi_step_device(self._h, stream))

    def fit(self, steps, check_interval=0):
        """`steps` steps (mi_vi_fit); returns their trace rows [steps][6] (TRACE_COLUMNS)."""
        out = np.empty((int(steps), 6))
        self._check(self._lib.mi_vi_fit(self._h, int(steps), int(check_interval), _ptr(out)))
        return out

    def trace(self, first_step=0, count=None):
        """Trace rows [first_step, first_step + count) of the steps so far (mi_vi_trace); count
        None: up to the last step."""
        if count is None:
            count = min(self.state().steps, self.max_steps) - int(first_step)
        out = np.empty((int(count), 6))
        self._check(self._lib.mi_vi_trace(self._h, int(first_step), int(count), _ptr(out)))
        return out

    def update(self, sbn_gradient, q_gradient, log_likelihoods, log_prior, log_q_topology, log_q_branch):
        """One update of the state from given gradients [P], [V][2] and the particles' terms [K]
        each (mi_vi_update).  Returns the trace row [6]."""
        P, V, K = self.parameter_count, self.variable_count, self.particle_count
        arrays = [_np(sbn_gradient, np.float64).reshape(P), _np(q_gradient, np.float64).reshape(V, 2)]
        arrays += [_np(x, np.float64).reshape(K) for x in (log_likelihoods, log_prior, log_q_topology, log_q_branch)]
        row = np.empty(6)
        self._check(self._lib.mi_vi_update(self._h, *[_ptr(x) for x in arrays], _ptr(row)))
        return row

    def update_device(self, stream, sbn_gradient, q_gradient, log_likelihoods, log_prior, log_q_topology,
                      log_q_branch, out_trace_row=None):
        """mi_vi_update_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_vi_update_device(self._h, stream, sbn_gradient, q_gradient, log_likelihoods,
                                                  log_prior, log_q_topology, log_q_branch, out_trace_row))

    def state(self):
        """The whole state (mi_vi_get_state): a ViState."""
        P, V = self.parameter_count, self.variable_count
        phi, q, ms, mq = np.empty(P), np.empty((V, 2)), np.empty((2, P)), np.empty((2, V, 2))
        scalars, counters = np.empty(5), np.empty(3, np.int64)
        self._check(self._lib.mi_vi_get_state(self._h, _ptr(phi), _ptr(q), _ptr(ms), _ptr(mq), _ptr(scalars),
                                              _ptr(counters)))
        return ViState(phi, q, ms, mq, float(scalars[0]), float(scalars[1]), scalars[2:4].copy(), float(scalars[4]),
                       int(counters[0]), int(counters[1]), int(counters[2]))

    def set_state(self, state):
        """Load a ViState (mi_vi_set_state): the fit goes on from it bit for bit."""
        P, V = self.parameter_count, self.variable_count
        phi, q = _np(state.log_params, np.float64).reshape(P), _np(state.q_params, np.float64).reshape(V, 2)
        ms, mq = _np(state.sbn_moments, np.float64).reshape(2, P), _np(state.q_moments, np.float64).reshape(2, V, 2)
        scalars = np.array([state.b0, state.b1, state.step_size[0], state.step_size[1], state.sbn_step_size])
        counters = np.array([state.steps, state.successes, state.first_sample], np.int64)
        self._check(self._lib.mi_vi_set_state(self._h, _ptr(phi), _ptr(q), _ptr(ms), _ptr(mq), _ptr(scalars),
                                              _ptr(counters)))

    def particles(self):
        """The last step's particles (mi_vi_particles): (parent ids [K][2n-3], branch lengths
        [K][2n-2], logL [K], log q of the topology [K], log q of the lengths [K], log prior [K])."""
        K, E = self.particle_count, 2 * self.taxon_count - 3
        pid, bl = np.empty((K, E), np.int32), np.empty((K, E + 1))
        ll, lqt, lqb, lp = np.empty(K), np.empty(K), np.empty(K), np.empty(K)
        self._check(self._lib.mi_vi_particles(self._h, _ptr(pid), _ptr(bl), _ptr(ll), _ptr(lqt), _ptr(lqb), _ptr(lp)))
        return pid, bl, ll, lqt, lqb, lp

    def estimate(self, particle_count, seed, first_sample=0):
        """The reference's estimate_elbo and marginal_likelihood_estimate (burrito.py:127-183) of
        the current state on fresh particles, composed from the engine's existing calls: returns
        (elbo, marginal likelihood estimate)."""
        e, K, T0 = self.engine, int(particle_count), self.support_ids.shape[0]
        st = self.state()
        sup = e.sbn_index(self.support_ids)
        pid, _, _, _ = e.sbn_sample(sup, e.sbn_descent(sup), st.log_params, K, seed, first_sample=first_sample)
        both = e.sbn_index(np.concatenate([self.support_ids, pid]), support_tree_count=T0)
        index = e.psp_index(both, e.psp_table(sup), rows=self.rows, trees=slice(T0, None))
        draw = e.branch_model_sample(index, st.q_params, seed, first_sample=first_sample,
                                     prior_rate=self.options.prior_rate)
        params = None if self.model_params is None else np.tile(self.model_params, (K, 1))
        ll = e.log_likelihoods(pid, draw.branch_lengths, params)
        _, lqt = e.sbn_log_prob(both, st.log_params, trees=slice(T0, None))
        f = ll + draw.log_prior - lqt - draw.log_q
        top = np.max(f)
        return float(np.mean(f)), float(top + np.log(np.sum(np.exp(f - top))) - np.log(K))


@dataclass
class GpStructure:
    """GeneralizedPruning.structure(): the subsplit DAG (include/mi_phylo.h, mi_gp_structure)."""
    taxon_count: int
    node_count: int
    rootsplit_count: int
    entry_count: int          # G
    pattern_count: int
    entries: np.ndarray       # [G][3] parent node, clade, child node; a rootsplit: (-1, -1, its node)
    block_range: np.ndarray   # [node_count][2][2] begin, end
    clades: np.ndarray        # [node_count][2][W] uint32 bitsets
    levels: np.ndarray        # [node_count] clade sizes
    topology_count: float


@dataclass
class GpLikelihoods:
    per_gpcsp_log_likelihood: np.ndarray   # [G]
    log_marginal: float
    pattern_log_marginal: np.ndarray = None  # [P] log M_p
    matrix: np.ndarray = None                # [G][P] log l_e per pattern


@dataclass
class GpBranchDerivatives:
    log_likelihood: np.ndarray   # [G] sum_p w_p log l_e
    derivative: np.ndarray       # [G] sum_p w_p l'_e / l_e
    gradient: np.ndarray         # [G] of log_marginal
    hessian: np.ndarray          # [G] its diagonal Hessian
    gsq: np.ndarray              # [G] S_e


@dataclass
class GpHybridRequests:
    formed: np.ndarray          # [G] bool: all four lists of the entry's request are non-empty
    first_summand: np.ndarray   # [G]
    summand_count: np.ndarray   # [G]
    summands: np.ndarray        # [S][4] the entries (rootward, sister, rotated, sorted) of every summand


@dataclass
class GpHybridMarginals:
    hybrid: np.ndarray     # [G]
    summands: np.ndarray   # [S]


@dataclass
class GpOptimizeResult:
    branch_lengths: np.ndarray   # [G] the last accepted point
    trace: np.ndarray            # the accepted log_marginal after each evaluation
    evaluations: int
    status: int                  # MI_BRANCH_OPT_*: 0 converged, 1 iteration limit, 2 stalled


@dataclass
class GpTreeIndex:
    """GeneralizedPruning.tree_index(): which entries and nodes of the DAG rooted trees use."""
    entries: np.ndarray   # [T][2n-1] per tree node the entry into it (the root: its rootsplit entry); G: not in the DAG
    nodes: np.ndarray     # [T][2n-1] the DAG node of every tree node; -1: not in the DAG


@dataclass
class GpTrees:
    """GeneralizedPruning.sample_trees() / enumerate_trees(): rooted trees built from the DAG."""
    parent_ids: np.ndarray       # [K][2n-2] leaves by taxon, post-order, children by largest leaf, root 2n-2
    entries: np.ndarray          # [K][2n-1] as tree_index gives them
    log_q: np.ndarray            # [K] as tree_log_prob gives it
    branch_lengths: np.ndarray   # [K][2n-1] the GP lengths b[entries], 0 at the root
    cdf: np.ndarray = None       # [G] the sampler's per-block running sums of q


@dataclass
class DerootedTrees:
    """Engine.deroot_trees()."""
    parent_ids: np.ndarray       # [T][2n-3]
    branch_lengths: np.ndarray   # [T][2n-2] or None
    root_edge: np.ndarray        # [T] the edge that carries the rooting
    new_id: np.ndarray = None    # [T][2n-1] deroot_trees_mapped: the unrooted edge of every rooted node's edge; the root: -1


@dataclass
class GpBranchDraw:
    """GeneralizedPruning.branch_sample(): branch lengths of rooted trees drawn per entry."""
    branch_lengths: np.ndarray   # [T][2n-1] theta; 0 in the root's slot
    epsilon: np.ndarray          # [T][2n-2]
    log_q: np.ndarray            # [T]
    log_prior: np.ndarray        # [T]


def gp_hybrid_request_count(parent_ids, max_summands=0):
    """(fully formed quartet hybrid requests, summands S) of the subsplit DAG that Engine.gp_create
    would build from rooted topologies parent_ids [T][2n-2] (mi_gp_hybrid_request_count).  Host
    arithmetic only, no engine.  Raises when S exceeds max_summands (0: the library's limit, 2^28,
    above which an object serves no hybrid call)."""
    pid = _np(parent_ids, np.int32)
    if pid.ndim != 2 or pid.shape[1] % 2:
        raise RuntimeError("gp_hybrid_request_count: parent_ids must be [T][2n-2]")
    formed, count = C.c_int32(), C.c_int64()
    if _capi.load().mi_gp_hybrid_request_count(pid.shape[0], pid.shape[1] // 2 + 1, _ptr(pid), int(max_summands),
                                               C.byref(formed), C.byref(count)):
        raise RuntimeError(_capi.last_error())
    return formed.value, count.value


class GeneralizedPruning:
    """Generalized pruning over a subsplit DAG (mi_gp, include/mi_phylo.h), made by
    Engine.gp_create.  The engine must outlive it."""

    def __init__(self, engine, handle):
        self.engine, self._h, self._lib = engine, handle, engine._lib
        sizes = np.zeros(8, np.int32)
        self._check(self._lib.mi_gp_sizes(self._h, sizes.ctypes.data_as(_capi.I32P)))
        (self.taxon_count, self.node_count, self.rootsplit_count, self.entry_count, self.pattern_count,
         self._words, self.level_count, self.tile_width) = (int(x) for x in sizes)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(_capi.last_error())

    def close(self):
        if self._h is not None:
            if self.engine._h is not None:
                self._lib.mi_gp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def structure(self):
        G, nodes = self.entry_count, self.node_count
        entries, block = np.empty((G, 3), np.int32), np.empty((nodes, 2, 2), np.int32)
        clades, levels = np.empty((nodes, 2, self._words), np.uint32), np.empty(nodes, np.int32)
        count = C.c_double()
        self._check(self._lib.mi_gp_structure(self._h, _ptr(entries), _ptr(block), _ptr(clades), _ptr(levels),
                                              C.byref(count)))
        return GpStructure(self.taxon_count, nodes, self.rootsplit_count, G, self.pattern_count, entries, block,
                           clades, levels, count.value)

    def strings(self):
        """The entries' names as GPInstance::PrettyIndexer gives them (mi_gp_strings)."""
        need = C.c_int64()
        self._check(self._lib.mi_gp_strings(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._check(self._lib.mi_gp_strings(self._h, buf, need.value, None))
        return buf.value.decode().split("\n")

    def set_branch_lengths(self, branch_lengths):
        b = _np(branch_lengths, np.float64).reshape(-1)
        self._check(self._lib.mi_gp_set_branch_lengths(self._h, _ptr(b), b.shape[0]))

    def get_branch_lengths(self):
        out = np.empty(self.entry_count)
        self._check(self._lib.mi_gp_get_branch_lengths(self._h, _ptr(out)))
        return out

    def set_sbn_parameters(self, q):
        q = _np(q, np.float64).reshape(-1)
        self._check(self._lib.mi_gp_set_sbn_parameters(self._h, _ptr(q), q.shape[0]))

    def get_sbn_parameters(self):
        out = np.empty(self.entry_count)
        self._check(self._lib.mi_gp_get_sbn_parameters(self._h, _ptr(out)))
        return out

    def node_probabilities(self, q):
        q, out = _np(q, np.float64).reshape(-1), np.empty(self.node_count)
        self._check(self._lib.mi_gp_node_probabilities(self._h, _ptr(q), q.shape[0], _ptr(out)))
        return out

    def inverted_probabilities(self, q):
        q, out = _np(q, np.float64).reshape(-1), np.empty(self.entry_count)
        self._check(self._lib.mi_gp_inverted_probabilities(self._h, _ptr(q), q.shape[0], _ptr(out)))
        return out

    def populate(self):
        """Both sweeps (mi_gp_populate: the reference's PopulatePLVs)."""
        self._check(self._lib.mi_gp_populate(self._h))

    def populate_device(self, stream=None):
        self._check(self._lib.mi_gp_populate_device(self._h, stream))

    def likelihoods(self, matrix=False, per_pattern=False):
        """mi_gp_likelihoods: a GpLikelihoods."""
        G, P = self.entry_count, self.pattern_count
        per, marg = np.empty(G), C.c_double()
        pat = np.empty(P) if per_pattern else None
        mat = np.empty((G, P)) if matrix else None
        self._check(self._lib.mi_gp_likelihoods(self._h, _ptr(per), C.byref(marg), _ptr(pat), _ptr(mat)))
        return GpLikelihoods(per, marg.value, pat, mat)

    def likelihoods_device(self, stream, out_per_gpcsp, out_log_marginal):
        """mi_gp_likelihoods_device: device pointers, enqueued on `stream`."""
        self._check(self._lib.mi_gp_likelihoods_device(self._h, stream, out_per_gpcsp, out_log_marginal))

    def components_of_full_log_marginal(self):
        """per_gpcsp_log_likelihood + site_count log q (GPEngine's components of the full marginal)."""
        w = self.engine._weights
        if w is None:
            raise RuntimeError("components_of_full_log_marginal needs the engine's pattern weights on the host")
        with np.errstate(divide="ignore"):
            return self.likelihoods().per_gpcsp_log_likelihood + float(np.sum(w)) * np.log(self.get_sbn_parameters())

    def branch_derivatives(self):
        """mi_gp_branch_derivatives: a GpBranchDerivatives."""
        G = self.entry_count
        pair, g, h, s = np.empty((G, 2)), np.empty(G), np.empty(G), np.empty(G)
        self._check(self._lib.mi_gp_branch_derivatives(self._h, _ptr(pair), _ptr(g), _ptr(h), _ptr(s)))
        return GpBranchDerivatives(pair[:, 0].copy(), pair[:, 1].copy(), g, h, s)

    def branch_derivatives_device(self, stream, out_ll_derivative, out_gradient, out_hessian, out_gsq):
        self._check(self._lib.mi_gp_branch_derivatives_device(self._h, stream, out_ll_derivative, out_gradient,
                                                              out_hessian, out_gsq))

    def estimate_sbn_parameters(self, hybrid=False):
        """mi_gp_estimate_sbn_parameters (the reference's EstimateSBNParameters); returns the new q.
        hybrid: mi_gp_estimate_sbn_parameters_hybrid, where a block whose entries all have a finite
        hybrid marginal takes softmax(hybrid + log q)."""
        out = np.empty(self.entry_count)
        call = self._lib.mi_gp_estimate_sbn_parameters_hybrid if hybrid else self._lib.mi_gp_estimate_sbn_parameters
        self._check(call(self._h, _ptr(out)))
        return out

    def hybrid_requests(self):
        """mi_gp_hybrid_requests: a GpHybridRequests (the quartet hybrid request of every entry)."""
        G, count = self.entry_count, C.c_int32()
        self._check(self._lib.mi_gp_hybrid_requests(self._h, None, None, C.byref(count)))
        req, summands = np.empty((G, 3), np.int32), np.empty((count.value, 4), np.int32)
        self._check(self._lib.mi_gp_hybrid_requests(self._h, _ptr(req), _ptr(summands), None))
        return GpHybridRequests(req[:, 0].astype(bool), req[:, 1].copy(), req[:, 2].copy(), summands)

    def reserve_hybrid(self):
        """mi_gp_reserve_hybrid: allocate what hybrid_marginals_device needs."""
        self._check(self._lib.mi_gp_reserve_hybrid(self._h))

    def hybrid_marginals(self, summands=False):
        """mi_gp_hybrid_marginals: hybrid [G] (-inf where the request is not fully formed); with
        summands=True a GpHybridMarginals that also holds every summand [S]."""
        out = np.empty(self.entry_count)
        if not summands:
            self._check(self._lib.mi_gp_hybrid_marginals(self._h, _ptr(out), None))
            return out
        count = C.c_int32()
        self._check(self._lib.mi_gp_hybrid_requests(self._h, None, None, C.byref(count)))
        each = np.empty(count.value)
        self._check(self._lib.mi_gp_hybrid_marginals(self._h, _ptr(out), _ptr(each)))
        return GpHybridMarginals(out, each)

    def hybrid_marginals_device(self, stream, out_hybrid, out_summands=None):
        """mi_gp_hybrid_marginals_device: device pointers, enqueued on `stream`; reads the last
        populate; needs reserve_hybrid() first."""
        self._check(self._lib.mi_gp_hybrid_marginals_device(self._h, stream, out_hybrid, out_summands))

    # ---- trees of the DAG ----
    def _trees(self, parent_ids):
        pid = _np(parent_ids, np.int32)
        if pid.ndim == 1:
            pid = pid[None, :]
        if pid.ndim != 2 or pid.shape[1] != 2 * self.taxon_count - 2:
            raise RuntimeError("parent_ids must be [T][2n-2]")
        return pid

    def _entries(self, entries):
        ent = _np(entries, np.int32)
        if ent.ndim == 1:
            ent = ent[None, :]
        if ent.ndim != 2 or ent.shape[1] != 2 * self.taxon_count - 1:
            raise RuntimeError("entries must be [T][2n-1]")
        return ent

    def reserve_trees(self, tree_capacity):
        """mi_gp_reserve_trees: upload the tree calls' tables, allocate workspace for tree_capacity trees."""
        self._check(self._lib.mi_gp_reserve_trees(self._h, int(tree_capacity)))

    def topology_count(self):
        """The DAG's topology count as an integer, saturated at 2^62 (mi_gp_topology_count)."""
        out = C.c_uint64()
        self._check(self._lib.mi_gp_topology_count(self._h, C.byref(out)))
        return out.value

    def tree_index(self, parent_ids):
        """mi_gp_tree_index: a GpTreeIndex of rooted trees parent_ids [T][2n-2]."""
        pid = self._trees(parent_ids)
        N = 2 * self.taxon_count - 1
        ent, nodes = np.empty((pid.shape[0], N), np.int32), np.empty((pid.shape[0], N), np.int32)
        self._check(self._lib.mi_gp_tree_index(self._h, pid.shape[0], _ptr(pid), _ptr(ent), _ptr(nodes)))
        return GpTreeIndex(ent, nodes)

    def tree_index_device(self, stream, T, parent_ids, out_entries, out_nodes=None):
        self._check(self._lib.mi_gp_tree_index_device(self._h, stream, T, parent_ids, out_entries, out_nodes))

    def tree_log_prob(self, entries):
        """mi_gp_tree_log_prob: log q [T] of indexed trees at the object's q (-inf at a sentinel)."""
        ent = self._entries(entries)
        out = np.empty(ent.shape[0])
        self._check(self._lib.mi_gp_tree_log_prob(self._h, ent.shape[0], _ptr(ent), _ptr(out)))
        return out

    def tree_log_prob_device(self, stream, T, entries, out_log_q):
        self._check(self._lib.mi_gp_tree_log_prob_device(self._h, stream, T, entries, out_log_q))

    def tree_branch_lengths(self, entries, missing_length=0.0):
        """mi_gp_tree_branch_lengths: [T][2n-1] the GP lengths of indexed trees."""
        ent = self._entries(entries)
        out = np.empty(ent.shape, np.float64)
        self._check(self._lib.mi_gp_tree_branch_lengths(self._h, ent.shape[0], _ptr(ent), float(missing_length), _ptr(out)))
        return out

    def tree_branch_lengths_device(self, stream, T, entries, missing_length, out_branch_lengths):
        self._check(self._lib.mi_gp_tree_branch_lengths_device(self._h, stream, T, entries, float(missing_length),
                                                               out_branch_lengths))

    def train_simple_average(self, entries, tree_weights=None):
        """mi_gp_train_simple_average (the rooted TrainSimpleAverage): sets and returns q [G]."""
        ent = self._entries(entries)
        w = None
        if tree_weights is not None:
            w = _np(tree_weights, np.float64).reshape(-1)
            if w.shape[0] != ent.shape[0]:
                raise RuntimeError("tree_weights must be [T]")
        out = np.empty(self.entry_count)
        self._check(self._lib.mi_gp_train_simple_average(self._h, ent.shape[0], _ptr(ent), _ptr(w), _ptr(out)))
        return out

    def _built(self, K, cdf):
        n = self.taxon_count
        return GpTrees(np.empty((K, 2 * n - 2), np.int32), np.empty((K, 2 * n - 1), np.int32), np.empty(K),
                       np.empty((K, 2 * n - 1)), np.empty(self.entry_count) if cdf else None)

    def sample_trees(self, sample_count, seed, first_sample=0, cdf=False):
        """mi_gp_sample_trees: a GpTrees of sample_count rooted trees drawn from q (Philox stream
        (seed, first_sample + k))."""
        t = self._built(int(sample_count), cdf)
        self._check(self._lib.mi_gp_sample_trees(self._h, int(sample_count), int(seed), int(first_sample), _ptr(t.parent_ids),
                                                 _ptr(t.entries), _ptr(t.log_q), _ptr(t.branch_lengths), _ptr(t.cdf)))
        return t

    def sample_trees_device(self, stream, K, seed, first_sample, out_parent_ids, out_entries, out_log_q,
                            out_branch_lengths=None, out_cdf=None):
        self._check(self._lib.mi_gp_sample_trees_device(self._h, stream, K, int(seed), int(first_sample), out_parent_ids,
                                                        out_entries, out_log_q, out_branch_lengths, out_cdf))

    def enumerate_trees(self, first=0, count=None):
        """mi_gp_enumerate_trees: a GpTrees of trees first .. first + count - 1 of the DAG (count None:
        all from `first` on)."""
        if count is None:
            count = self.topology_count() - int(first)
        t = self._built(int(count), False)
        self._check(self._lib.mi_gp_enumerate_trees(self._h, int(first), int(count), _ptr(t.parent_ids), _ptr(t.entries),
                                                    _ptr(t.log_q), _ptr(t.branch_lengths)))
        return t

    def enumerate_trees_device(self, stream, first, count, out_parent_ids, out_entries, out_log_q,
                               out_branch_lengths=None):
        self._check(self._lib.mi_gp_enumerate_trees_device(self._h, stream, int(first), int(count), out_parent_ids,
                                                           out_entries, out_log_q, out_branch_lengths))

    # ---- the variational fit over the DAG's rooted trees ----
    def reserve_vi(self, tree_capacity):
        """mi_gp_reserve_vi: the workspace of the calls below for tree_capacity trees (reserve_trees included)."""
        self._check(self._lib.mi_gp_reserve_vi(self._h, int(tree_capacity)))

    def log_normalize(self, log_params):
        """mi_gp_log_normalize: (log q [G], q [G]) of unnormalised log parameters, normalised per block."""
        phi = _np(log_params, np.float64).reshape(self.entry_count)
        lq, q = np.empty(self.entry_count), np.empty(self.entry_count)
        self._check(self._lib.mi_gp_log_normalize(self._h, _ptr(phi), _ptr(lq), _ptr(q)))
        return lq, q

    def log_normalize_device(self, stream, log_params, out_log_q, out_q):
        self._check(self._lib.mi_gp_log_normalize_device(self._h, stream, log_params, out_log_q, out_q))

    def branch_sample(self, entries, q_params, seed, first_sample=0, prior_rate=10.0, epsilon=None):
        """mi_gp_branch_sample: a GpBranchDraw of the trees given by entries [T][2n-1], one log-normal
        variable (mu, sigma) = q_params[e] per entry; epsilon [T][2n-2] replaces the Philox normals."""
        ent = self._entries(entries)
        T, N = ent.shape
        q = _np(q_params, np.float64).reshape(self.entry_count, 2)
        eps = None if epsilon is None else _np(epsilon, np.float64).reshape(T, N - 1)
        d = GpBranchDraw(np.empty((T, N)), np.empty((T, N - 1)), np.empty(T), np.empty(T))
        self._check(self._lib.mi_gp_branch_sample(self._h, T, _ptr(ent), _ptr(q), int(seed) & (2 ** 64 - 1), int(first_sample),
                                                  float(prior_rate), _ptr(eps), _ptr(d.branch_lengths), _ptr(d.epsilon),
                                                  _ptr(d.log_q), _ptr(d.log_prior)))
        return d

    def branch_sample_device(self, stream, T, entries, q_params, seed, first_sample, prior_rate, epsilon_in,
                             out_branch_lengths, out_epsilon, out_log_q, out_log_prior):
        self._check(self._lib.mi_gp_branch_sample_device(self._h, stream, T, entries, q_params, int(seed) & (2 ** 64 - 1),
                                                         int(first_sample), float(prior_rate), epsilon_in, out_branch_lengths,
                                                         out_epsilon, out_log_q, out_log_prior))

    def branch_gradient(self, entries, q_params, draw, new_id, branch_gradient, log_likelihoods, log_q_topology=None,
                        tree_weights=None, beta=1.0, prior_rate=10.0):
        """mi_gp_branch_gradient: (gradient [G][2] with respect to q_params, log_f [T]) from a
        GpBranchDraw, the mapped de-rooting's new_id [T][2n-1] and the unrooted gradient call's
        branch gradient [T][2n-1] and log-likelihoods [T] of the de-rooted trees."""
        ent = self._entries(entries)
        T, N = ent.shape
        q = _np(q_params, np.float64).reshape(self.entry_count, 2)
        arrays = [_np(draw.branch_lengths, np.float64).reshape(T, N), _np(draw.epsilon, np.float64).reshape(T, N - 1),
                  _np(draw.log_q, np.float64).reshape(T), _np(draw.log_prior, np.float64).reshape(T),
                  _np(new_id, np.int32).reshape(T, N), _np(branch_gradient, np.float64).reshape(T, N),
                  _np(log_likelihoods, np.float64).reshape(T)]
        lqt = None if log_q_topology is None else _np(log_q_topology, np.float64).reshape(T)
        w = None if tree_weights is None else _np(tree_weights, np.float64).reshape(T)
        out, log_f = np.empty((self.entry_count, 2)), np.empty(T)
        self._check(self._lib.mi_gp_branch_gradient(self._h, T, _ptr(ent), _ptr(q), *[_ptr(x) for x in arrays], _ptr(lqt),
                                                    _ptr(w), float(beta), float(prior_rate), _ptr(out), _ptr(log_f)))
        return out, log_f

    def branch_gradient_device(self, stream, T, entries, q_params, branch_lengths, epsilon, log_q_branch, log_prior,
                               new_id, branch_gradient, log_likelihoods, log_q_topology, tree_weights, beta, prior_rate,
                               out_gradient, out_log_f):
        self._check(self._lib.mi_gp_branch_gradient_device(self._h, stream, T, entries, q_params, branch_lengths, epsilon,
                                                           log_q_branch, log_prior, new_id, branch_gradient,
                                                           log_likelihoods, log_q_topology, tree_weights, float(beta),
                                                           float(prior_rate), out_gradient, out_log_f))

    def topology_gradient(self, entries, log_params, log_f, estimator="vimco"):
        """mi_gp_topology_gradient: (gradient [G] with respect to log_params, factors [T])."""
        ent = self._entries(entries)
        T = ent.shape[0]
        phi, f = _np(log_params, np.float64).reshape(self.entry_count), _np(log_f, np.float64).reshape(T)
        out, factors = np.empty(self.entry_count), np.empty(T)
        self._check(self._lib.mi_gp_topology_gradient(self._h, T, _ptr(ent), _ptr(phi), _ptr(f), _SBN_FACTORS[estimator],
                                                      _ptr(out), _ptr(factors)))
        return out, factors

    def topology_gradient_device(self, stream, T, entries, log_params, log_f, estimator, out_gradient, out_factors=None):
        self._check(self._lib.mi_gp_topology_gradient_device(self._h, stream, T, entries, log_params, log_f,
                                                             _SBN_FACTORS[estimator], out_gradient, out_factors))

    def default_q_params(self):
        """The mode match of the object's b: sigma = -0.1 log clip(b, 1e-6, 1 - 1e-6), mu = sigma^2 +
        log max(b, 1e-6); the rootsplit rows, which no edge draws from, are (0, 1)."""
        b = self.get_branch_lengths()[:self.entry_count]
        sigma = -0.1 * np.log(np.clip(b, 1e-6, 1.0 - 1e-6))
        q = np.stack([sigma * sigma + np.log(np.maximum(b, 1e-6)), sigma], axis=1)
        q[:self.rootsplit_count] = (0.0, 1.0)
        return q

    def vi_create(self, log_params=None, q_params=None, model_params=None, particle_count=10, estimator="vimco",
                  anneal_steps=0, max_steps=1000, prior_rate=10.0, step_size=(0.001, 0.001), sbn_step_size=0.001,
                  step_decay=0.99, adam_beta0=0.9, adam_beta1=0.999, adam_epsilon=1e-8, seed=0, first_sample=0, rows=1):
        """A device-resident variational fit over the rooted trees of this DAG (mi_gp_vi_create;
        DESIGN.md 4.29).  log_params [G] defaults to the log of the object's q, q_params [G][2] to
        default_q_params(); model_params: the one parameter row every particle takes.  Returns a
        RootedVariationalFit."""
        if estimator not in ("plain", "vimco"):
            raise RuntimeError(f"vi_create: estimator must be 'plain' or 'vimco', got {estimator!r}")
        e = self.engine
        if log_params is None:
            with np.errstate(divide="ignore"):
                log_params = np.log(self.get_sbn_parameters())
        if q_params is None:
            q_params = self.default_q_params()
        phi, q = _np(log_params, np.float64).reshape(-1), _np(q_params, np.float64).reshape(-1, 2)
        mp = None if model_params is None or e.param_count == 0 else _np(model_params, np.float64).reshape(e.param_count)
        o = _capi.ViOptions()
        self._check(self._lib.mi_vi_default_options(C.byref(o)))
        o.particle_count, o.rows, o.estimator = int(particle_count), int(rows), _SBN_FACTORS[estimator]
        o.anneal_steps, o.max_steps, o.prior_rate = int(anneal_steps), int(max_steps), float(prior_rate)
        o.step_size[0], o.step_size[1] = (float(x) for x in np.broadcast_to(step_size, 2))
        o.sbn_step_size, o.step_decay = float(sbn_step_size), float(step_decay)
        o.adam_beta0, o.adam_beta1, o.adam_epsilon = float(adam_beta0), float(adam_beta1), float(adam_epsilon)
        o.seed, o.first_sample = int(seed) & (2 ** 64 - 1), int(first_sample)
        h = C.c_void_p()
        self._check(self._lib.mi_gp_vi_create(self._h, _ptr(mp), phi.shape[0], _ptr(phi), q.shape[0], _ptr(q), C.byref(o),
                                              C.byref(h)))
        return RootedVariationalFit(self, h, mp, o)

    def optimize_branch_lengths(self, tolerance=1e-6, max_iterations=100, min_length=np.exp(-13.9),
                                max_length=np.exp(1.1), check_interval=4):
        """Maximise log_marginal over all branch lengths (mi_gp_optimize_branch_lengths): a
        GpOptimizeResult."""
        o = _branch_opt_options(max_iterations, check_interval, 0, tolerance, min_length, max_length)
        trace = np.empty(max(int(max_iterations), 1))
        evals, status = C.c_int32(), C.c_int32()
        self._check(self._lib.mi_gp_optimize_branch_lengths(self._h, C.byref(o), _ptr(trace), C.byref(evals),
                                                            C.byref(status)))
        return GpOptimizeResult(self.get_branch_lengths(), trace[:evals.value].copy(), evals.value, status.value)


class RootedVariationalFit(VariationalFit):
    """A variational fit over the rooted trees of a subsplit DAG (mi_gp_vi_create),
    made by GeneralizedPruning.vi_create.  step_device, fit, trace, update, state and set_state are
    VariationalFit's.  The object and its engine must outlive it."""

    def __init__(self, gp, handle, model_params, options):
        super().__init__(gp.engine, handle, None, model_params, options)
        self.gp = gp

    def particles(self):
        """The last step's rooted particles (mi_gp_vi_particles): (parent ids [K][2n-2], entries
        [K][2n-1], branch lengths [K][2n-1], logL [K], log q of the topology [K], log q of the
        lengths [K], log prior [K])."""
        K, N = self.particle_count, 2 * self.taxon_count - 1
        pid, ent, bl = np.empty((K, N - 1), np.int32), np.empty((K, N), np.int32), np.empty((K, N))
        ll, lqt, lqb, lp = np.empty(K), np.empty(K), np.empty(K), np.empty(K)
        self._check(self._lib.mi_gp_vi_particles(self._h, _ptr(pid), _ptr(ent), _ptr(bl), _ptr(ll), _ptr(lqt), _ptr(lqb),
                                                 _ptr(lp)))
        return pid, ent, bl, ll, lqt, lqb, lp

    def export(self):
        """(normalised q [G], exp(mu - sigma^2) [G]) of the current state, in plain Python: what
        set_sbn_parameters and set_branch_lengths of the object take (the mode of every entry's
        log-normal as its branch length)."""
        st = self.state()
        s = self.gp.structure()
        blocks = [(0, s.rootsplit_count)] + [tuple(int(x) for x in s.block_range[v, c])
                                             for v in range(s.taxon_count, s.node_count) for c in range(2)]
        q = np.zeros(s.entry_count)
        for lo, hi in blocks:
            phi = st.log_params[lo:hi]
            top = np.max(phi) if hi > lo else 0.0
            if np.isfinite(top):
                w = np.exp(phi - top)
                q[lo:hi] = w / np.sum(w)
        return q, np.exp(st.q_params[:, 0] - st.q_params[:, 1] ** 2)

    def estimate(self, particle_count, seed, first_sample=0):
        """(elbo, marginal likelihood estimate) of the current state on fresh particles, composed from
        the by-value calls.  Unlike a step of the fit, which never touches the object, this draws
        through sample_trees: the object's own q is set to the state's for the draw and put back
        (set_sbn_parameters), which leaves a full object's vectors stale: populate() again before
        its likelihood calls.  A DAG-only object has no vectors to go stale."""
        g, e, K = self.gp, self.engine, int(particle_count)
        st = self.state()
        _, q = g.log_normalize(st.log_params)
        kept = g.get_sbn_parameters()
        g.set_sbn_parameters(q)
        try:
            trees = g.sample_trees(K, seed, first_sample=first_sample)
        finally:
            g.set_sbn_parameters(kept)
        draw = g.branch_sample(trees.entries, st.q_params, seed, first_sample=first_sample,
                               prior_rate=self.options.prior_rate)
        un = e.deroot_trees(trees.parent_ids, draw.branch_lengths)
        params = None if self.model_params is None else np.tile(self.model_params, (K, 1))
        ll = e.log_likelihoods(un.parent_ids, un.branch_lengths, params)
        f = ll + draw.log_prior - trees.log_q - draw.log_q
        top = np.max(f)
        return float(np.mean(f)), float(top + np.log(np.sum(np.exp(f - top))) - np.log(K))


class DevicePatterns:
    """The compressed alignment left on the device (mi_site_pattern_compress_device): device
    pointers of the int32 [taxon][pattern] matrix and the float64 weights; `as_device_tips()`
    is what Engine(device_tips=...) takes; freed with mi_device_free when released."""

    def __init__(self, patterns_ptr, weights_ptr, taxon_count, pattern_count):
        self.patterns_ptr, self.weights_ptr = patterns_ptr, weights_ptr
        self.taxon_count, self.pattern_count = taxon_count, pattern_count

    def as_device_tips(self):
        return (self.patterns_ptr, self.weights_ptr, self.taxon_count, self.pattern_count)

    def release(self):
        lib = _capi.load()
        for ptr in (self.patterns_ptr, self.weights_ptr):
            if ptr:
                lib.mi_device_free(C.c_void_p(ptr))
        self.patterns_ptr = self.weights_ptr = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def site_pattern_compress_device(codes, device=0, keep_on_device=False):
    """SitePattern::Compress on the GPU (include/mi_phylo.h: mi_site_pattern_compress).

    codes: [taxon][site] symbol codes 0..3, 4 = gap / ambiguous.  Returns (patterns
    [taxon][P] int32, weights [P] float64, milliseconds of the column-hashing kernel) in
    the reference's pattern order; keep_on_device=True: (DevicePatterns, milliseconds) -- the
    matrix and the weights stay in device memory (mi_site_pattern_compress_device)."""
    lib = _capi.load()
    c = _np(codes, np.int8)
    n, L = c.shape
    if keep_on_device:
        count, ms = C.c_int32(0), C.c_double(0.0)
        d_pat, d_w = C.c_void_p(), C.c_void_p()
        if lib.mi_site_pattern_compress_device(int(device), n, L, _ptr(c), C.byref(count),
                                               C.byref(d_pat), C.byref(d_w), C.byref(ms)):
            raise RuntimeError(_capi.last_error())
        return DevicePatterns(d_pat.value, d_w.value, n, count.value), ms.value
    patterns = np.empty((n, L), dtype=np.int32)
    weights = np.empty(L, dtype=np.float64)
    count = C.c_int32(0)
    ms = C.c_double(0.0)
    if lib.mi_site_pattern_compress(int(device), n, L, _ptr(c), C.byref(count), _ptr(patterns),
                                    _ptr(weights), C.byref(ms)):
        raise RuntimeError(_capi.last_error())
    P = count.value
    return patterns.reshape(-1)[:n * P].reshape(n, P).copy(), weights[:P].copy(), ms.value
