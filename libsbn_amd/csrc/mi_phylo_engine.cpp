// Host side of the C ABI declared in include/mi_phylo.h: engine creation and destruction
// (device memory), error reporting, status, profiling and the device-pointer entry points (the
// call sequences behind them: mi_phylo_call.cpp).  Compiled with hipcc; no torch.
#include <map>
#include <memory>

#include "mi_phylo_engine.h"
#include "mi_phylo_tip_forms.h"

namespace {
thread_local std::string g_error;
}

namespace miphylo {
// sets mi_last_error(); shared with mi_site_pattern.hip
int fail(const std::string& msg) {
  g_error = msg;
  return 1;
}
void set_last_error(const std::string& msg) { g_error = msg; }
std::atomic<int64_t> device_bytes_held{0};
}  // namespace miphylo

// (what the members do after this body: mi_phylo_engine.h)
mi_engine::~mi_engine() {
  for (mi_engine* shard : shards) delete shard;
  if (!stream) return;
  (void)hipSetDevice(spec.device);
  (void)hipStreamSynchronize(stream);
}

namespace {
// (engine creation, tips in mask form on the device: the log-likelihood kernel's pre-tiled copy)
int build_tip_tiles(mi_engine* e) {
  e->tile_regs = engine_tile_regs(e);
  if (e->s == kStates) {  // which patterns carry no information (the per-pattern call reports them as exactly 0)
    if (e->pattern_blank.ensure((size_t)e->P)) return 1;
    launch_pattern_blank(e->have_tip_masks ? e->tip_masks.as<uint8_t>() : nullptr, e->tip_partials.as<double>(), e->n,
                         e->P, e->pattern_blank.as<uint8_t>(), e->stream);
  }
  if (!e->have_tip_masks || e->K > kMaxCategories) return 0;
  if (e->tip_tiles.ensure(loglik_tip_tiles_bytes(e->n, e->P, e->K))) return 1;
  launch_tip_tiles(e->tip_masks.as<uint8_t>(), e->tip_tiles.as<uint8_t>(), e->n, e->P, e->K, e->stream);
  // ... and the look-up walk's, for the engine's tile width
  if (walk3_possible(e) && gradient_mfma_groups(e->K) == 1) {
    const int regs = e->tile_regs;
    if (e->tip_code_tiles.ensure(tip_code_tiles_bytes(e->n, e->P, e->K, regs))) return 1;
    launch_tip_code_tiles(e->tip_codes.as<uint8_t>(), e->tip_code_tiles.as<uint8_t>(), e->n, e->P, e->K, regs, e->stream);
  }
  return 0;
}
template <typename T>
int upload(Buffer& b, const T* host, size_t count, hipStream_t s) {
  if (b.ensure(sizeof(T) * std::max<size_t>(count, 1))) return 1;
  if (count) HIP_TRY(hipMemcpyAsync(b.ptr, host, sizeof(T) * count, hipMemcpyHostToDevice, s));
  return 0;
}

// ---- engine creation: create_engine below, step by step ----

// A new engine's tips and pattern weights: host arrays, or (on_device:
// mi_engine_create_device_tips) states and weights already on the engine's device.
struct TipSource {
  const int32_t* states;
  const double* partials;
  const double* weights;
  bool on_device = false;
};
// What prepare_tips uploads asynchronously: create_engine keeps it until its one synchronisation.
struct TipStaging {
  Buffer states;                       // the caller's host states, for tips_prepare_kernel
  std::vector<int32_t> from_partials;  // 20 states: the compact states of the caller's partials
  std::vector<uint8_t> masks, codes;   // 4 states: the forms of the caller's partials
};

// The switches of a new engine (or sharded handle), read before anything else is done.
int32_t read_switches(Switches& sw) {
  std::string error;
  return parse_switches(sw, error) ? 0 : fail(error);
}

int check_spec(const mi_engine_spec* spec, const TipSource& t) {
  if (spec->taxon_count < 3) return fail("need at least 3 taxa");
  if (spec->pattern_count < 1) return fail("need at least one site pattern");
  if (spec->state_count != kStates && spec->state_count != kAa)
    return fail("state_count must be 4 (DNA, as in the reference: substitution_model.cpp:6-15) "
                "or 20 (amino acids)");
  const int states = spec->state_count;
  if (states == kStates && spec->subst_model != MI_SUBST_JC69 && spec->subst_model != MI_SUBST_GTR)
    return fail("Substitution model not known");
  if (states == kAa && spec->subst_model != MI_SUBST_REVERSIBLE)
    return fail("a 20-state engine takes subst_model MI_SUBST_REVERSIBLE (an empirical model "
                "given as data; WAG when none is passed)");
  if (spec->site_model != MI_SITE_CONSTANT && spec->site_model != MI_SITE_WEIBULL)
    return fail("Site model not known");
  if (spec->clock_model != MI_CLOCK_NONE && spec->clock_model != MI_CLOCK_STRICT)
    return fail("Clock model not known");
  if (spec->site_model == MI_SITE_CONSTANT && spec->category_count != 1)
    return fail("the constant site model has exactly one rate category");
  if (spec->category_count < 1 || spec->category_count > kMaxCategories)
    return fail("category_count out of range (1..64)");
  if (!t.states && !(spec->use_tip_states == 0 && t.partials)) return fail("tip_states is required");
  if (!t.weights) return fail("pattern_weights is required");
  const int count = mi_device_count();
  if (count == 0) return fail("no HIP device available: the MI355X engine has no CPU fallback");
  if (spec->device >= count) return fail("device ordinal out of range");
  return 0;
}

// the engine's sizes (its device is current)
void set_shape(mi_engine* e, const Switches& sw) {
  const mi_engine_spec& spec = e->spec;
  e->n = spec.taxon_count;
  e->N = 2 * e->n - 1;
  e->P = spec.pattern_count;
  e->K = spec.category_count;
  e->s = spec.state_count;
  if (e->s == kAa) {
    e->tiles = aa_tiles(e->P);
    e->ll_stride = aa_ll_blocks(e->P);
    // 32 MB per vector at 50 000 patterns x 4 categories, 16.4 GB per gradient tree of 512
    // taxa: the arena gets half of what the device has free now (an MI355X has 288 GB; more
    // trees per launch fill its 256 CUs better: 8 such trees in one launch instead of 3 + 3 + 2
    // are 8 % quicker), never less than 8 GB; aa_reserve backs off if that cannot be had
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)96 << 30;
    e->plv_budget = std::max<size_t>(free_b / 2, (size_t)8 << 30);
  } else {
    e->tiles = (e->P + kTile - 1) / kTile;
    e->ll_stride =
        std::max({e->tiles, loglik_mfma_tiles(e->P, e->K), gradient_mfma_tiles(e->P, e->K)});
  }
  int lg = 0;
  while ((2 << lg) <= e->n) lg++;
  e->max_slots = lg + 1;
  e->sw = sw;
  e->fused_setup = sw.fused_setup;
  if (sw.plv_bytes >= 0) e->plv_budget = (size_t)sw.plv_bytes;
}

// BlockSpecification (block_specification.cpp:11-50, phylo_model.cpp:13-15): names in map order
void set_blocks(mi_engine* e) {
  std::map<std::string, std::pair<int, int>> bm;
  int off = 0;
  auto block = [&](const char* name, int length) {  // the next `length` parameters; returns their start
    bm[name] = {off, length};
    off += length;
    return off - length;
  };
  e->rates_off = e->freqs_off = e->shape_off = e->clock_off = -1;
  if (e->spec.subst_model == MI_SUBST_GTR) {
    e->rates_off = block("GTR rates", 6);
    e->freqs_off = block("frequencies", 4);
  }
  bm["entire substitution"] = {0, off};
  const int site_start = off;
  if (e->spec.site_model == MI_SITE_WEIBULL) e->shape_off = block("Weibull shape", 1);
  bm["entire site"] = {site_start, off - site_start};
  const int clock_start = off;
  if (e->spec.clock_model == MI_CLOCK_STRICT) e->clock_off = block("clock rate", 1);
  bm["entire clock"] = {clock_start, off - clock_start};
  bm["entire"] = {0, off};
  e->param_count = off;
  for (const auto& kv : bm) e->blocks.push_back({kv.first, kv.second.first, kv.second.second});
}

int start_stream(mi_engine* e) {
  if (hipStreamCreateWithFlags(&e->stream.h, hipStreamNonBlocking) != hipSuccess)
    return fail("hipStreamCreate failed");
  if (e->status.ensure(sizeof(int32_t) * kStatusWords) ||
      hipMemsetAsync(e->status.ptr, 0, sizeof(int32_t) * kStatusWords, e->stream) != hipSuccess)
    return fail("status word allocation failed");
  if (e->spec.site_model == MI_SITE_WEIBULL) {
    // what the Weibull site model needs of its quantiles, once per engine (kernels_setup.hip)
    if (e->weibull_x.ensure(sizeof(double) * 2 * (size_t)e->K)) return 1;
    launch_weibull_table(e->K, e->weibull_x.as<double>(), e->stream);
  }
  return 0;
}

// Everything engine creation derives from the compact tip states (mi_phylo_tip_forms.h), on the
// device: the int8 states (rows padded with gaps to `stride`), and for 4-state engines the state
// masks, the table offsets of the third-generation walk and (use_tip_states == 0) the 0/1
// partial vectors of SitePattern::GetPartials (site_pattern.cpp:117-131).
__global__ __launch_bounds__(256) void tips_prepare_kernel(const int32_t* in, int n, int P, int states,
                                                           int stride, int8_t* st8, uint8_t* masks,
                                                           uint8_t* codes, double* partials) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * stride) return;
  const int x = (int)(idx / stride), p = (int)(idx - (size_t)x * stride);
  const size_t i = (size_t)x * P + p;
  const int c = p < P ? tip_state(in[i], states) : states;
  st8[idx] = (int8_t)c;
  if (p >= P) return;
  if (masks) masks[i] = tip_mask(c);
  if (codes) codes[i] = tip_code(c);
  if (partials)
    for (int k = 0; k < kStates; k++) partials[i * kStates + k] = tip_partial(c, k);
}

// Compact states, the caller's on either side or (20 states) those of the caller's partials, go
// through the kernel; the host derives only the forms of caller-supplied 4-state partials.
int prepare_tips(mi_engine* e, const TipSource& t, TipStaging& st) {
  const int states = e->s, n = e->n, P = e->P;
  const bool dna = states == kStates;
  const size_t np = (size_t)n * P;
  // (the two arrays must be device memory of THIS engine's device: a host pointer or another
  // device's memory would fault inside the preparation kernel, or worse, not fault)
  if (t.on_device)
    for (const void* p : {static_cast<const void*>(t.states), static_cast<const void*>(t.weights)}) {
      hipPointerAttribute_t at{};
      if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice ||
          at.device != e->spec.device) {
        (void)hipGetLastError();
        return fail("device_tip_states / device_pattern_weights must be device memory of "
                    "the engine's device");
      }
    }
  const double* partials = e->spec.use_tip_states ? nullptr : t.partials;
  const int32_t* d_states = t.states;  // (on the host until uploaded)
  if (partials && !dna) {
    // the 20-state kernels read compact states only; tip partials are accepted in the form
    // SitePattern::GetPartials produces (one-hot, or all ones for a gap: site_pattern.cpp:117-131)
    st.from_partials.resize(np);
    for (size_t i = 0; i < np; i++)
      if ((st.from_partials[i] = tip_state_of_partials(partials + i * states, states)) < 0)
        return fail("20-state engine: tip partials must be one-hot or all ones");
    d_states = st.from_partials.data();
  }
  if (d_states && !t.on_device) {
    if (upload(st.states, d_states, np, e->stream)) return 1;
    d_states = st.states.as<int32_t>();
  }
  // 20 states: rows padded with gaps to whole 16-pattern tiles (the walk kernels read them
  // unmasked), and a tile group of slack behind the last row (the workgroup kernels fetch the
  // states of their whole pattern range, padding waves included, with one LDS-DMA)
  const int stride = dna ? P : e->tiles * kAaTile;
  const size_t rows = (size_t)n * stride, slack = dna ? 0 : kAaTipSlack;
  // 4 states: masks, codes and (use_tip_states == 0) partial rows follow from the states unless
  // the caller brought partials.  (codes + 16 bytes: the look-up walk reads 12-byte groups as
  // three words.)
  const bool derive = dna && !partials;
  if (e->tip_states.ensure(rows + slack)) return 1;
  if (derive && (e->tip_masks.ensure(np) || e->tip_codes.ensure(np + 16))) return 1;
  if (derive && !e->spec.use_tip_states && e->tip_partials.ensure(sizeof(double) * np * kStates)) return 1;
  // (gaps wherever the kernel does not write: the slack, every state of an engine made from partials alone)
  HIP_TRY(hipMemsetAsync(e->tip_states.ptr, states, rows + slack, e->stream));
  if (derive) HIP_TRY(hipMemsetAsync(e->tip_codes.ptr, 64, np + 16, e->stream));
  if (d_states)
    hipLaunchKernelGGL(tips_prepare_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, e->stream,
                       d_states, n, P, states, stride, e->tip_states.as<int8_t>(),
                       derive ? e->tip_masks.as<uint8_t>() : nullptr, derive ? e->tip_codes.as<uint8_t>() : nullptr,
                       derive && !e->spec.use_tip_states ? e->tip_partials.as<double>() : nullptr);
  e->have_tip_masks = e->have_tip_codes = derive;
  if (!dna || derive) return 0;
  // The caller's 4-state partials are kept as they are.  They have state masks (the matrix-core
  // kernels) when every entry is exactly 0 or 1 -- real-valued partials take the HBM-streamed
  // kernel -- and codes (the look-up walk, kernels_walk3.hip) when every vector is one of the
  // five SitePattern produces; an engine with any other 0/1 vector keeps the mask kernels.
  if (upload(e->tip_partials, partials, np * kStates, e->stream)) return 1;
  st.masks.resize(np);
  st.codes.assign(np + 16, 64);
  e->have_tip_masks = e->have_tip_codes = true;
  for (size_t i = 0; i < np && e->have_tip_masks; i++) {
    st.masks[i] = tip_mask_of_partials(partials + i * kStates);
    st.codes[i] = tip_code_of_mask(st.masks[i]);
    e->have_tip_masks = st.masks[i] != kTipNoForm;
    e->have_tip_codes &= st.codes[i] != kTipNoForm;  // (no mask: no code either)
  }
  if (e->have_tip_masks && upload(e->tip_masks, st.masks.data(), np, e->stream)) return 1;
  if (e->have_tip_codes && upload(e->tip_codes, st.codes.data(), np + 16, e->stream)) return 1;
  return 0;
}

// what follows the tip forms, whichever side they came from, and creation's one synchronisation
int finish_tips(mi_engine* e, const TipSource& t, const double* exchangeabilities, const double* frequencies) {
  if (build_tip_tiles(e)) return 1;
  if (e->s == kAa && aa_engine_init(e, exchangeabilities, frequencies)) return 1;
  const size_t bytes = sizeof(double) * (size_t)e->P;
  if (e->weights.ensure(bytes) ||
      hipMemcpyAsync(e->weights.ptr, t.weights, bytes,
                     t.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream) != hipSuccess)
    return fail("copy of the pattern weights failed");
  if (hipStreamSynchronize(e->stream) != hipSuccess || hipGetLastError() != hipSuccess)
    return fail("preparation of the tips failed");
  return 0;
}

// A failed step returns at once: the engine, and with it whatever it had allocated, goes with `e`.
int32_t create_engine(const mi_engine_spec* spec, const Switches& sw, const double* exchangeabilities,
                      const double* frequencies, const TipSource& tips, mi_engine** out_engine) {
  if (!spec || !out_engine) return fail("null spec / out_engine");
  *out_engine = nullptr;
  if (check_spec(spec, tips)) return 1;
  if (spec->device >= 0) HIP_TRY(hipSetDevice(spec->device));
  TipStaging staging;  // (before `e`: a failed engine synchronises its stream before the staging goes)
  std::unique_ptr<mi_engine> e(new mi_engine());
  e->spec = *spec;
  if (spec->device < 0) HIP_TRY(hipGetDevice(&e->spec.device));
  set_shape(e.get(), sw);
  set_blocks(e.get());
  if (start_stream(e.get()) || prepare_tips(e.get(), tips, staging) ||
      finish_tips(e.get(), tips, exchangeabilities, frequencies))
    return 1;
  *out_engine = e.release();
  return 0;
}

// columns [b, b + c) of a host array [taxon][pattern][width] (a pattern shard's tips)
template <typename T>
const T* slice_columns(const T* all, int n, int P, int b, int c, int width, std::vector<T>& store) {
  if (!all) return nullptr;
  store.resize((size_t)n * c * width);
  for (int x = 0; x < n; x++)
    std::copy(all + ((size_t)x * P + b) * width, all + ((size_t)x * P + b + c) * width,
              store.begin() + (size_t)x * c * width);
  return store.data();
}

}  // namespace

int check_status(mi_engine* e, hipStream_t s) {
  HIP_TRY(hipSetDevice(e->spec.device));
  int32_t st[kStatusWords] = {};
  HIP_TRY(hipMemcpyAsync(st, e->status.ptr, sizeof st, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (st[2] != 0) {
    // A walk wave of the one-launch call waited in vain for its tree's set-up waves (workgroups
    // not dispatched in id order? the device held by another process's kernels for longer than
    // the poll's budget?).  The time-out has a status word of its own, so that an input error
    // in the same batch -- status[0] keeps the FIRST code -- cannot hide it.  This engine takes
    // the four-launch sequence from now on (a hipGraph captured BEFORE this point still replays
    // the one-launch kernel: re-capture it); a host-pointer entry point runs the call again at
    // once and returns its results (finish_host), a *_device caller gets the message
    // below.  (reduce_finalize has cleared every tree's hand-off word already; the memset makes
    // the "zero between calls" invariant independent of that.)
    e->fused_setup = false;
    e->fused_timed_out = true;
    if (e->ready.ptr) HIP_TRY(hipMemsetAsync(e->ready.ptr, 0, e->ready.bytes, s));
    if (st[0] == 0) {
      st[0] = kFusedTimeout;
      st[1] = st[2] - 1;
    }
  }
  if (st[0] != 0) {  // reported once: the first error since the last check
    HIP_TRY(hipMemsetAsync(e->status.ptr, 0, sizeof(int32_t) * kStatusWords, s));
    HIP_TRY(hipStreamSynchronize(s));
    // (a shard of a sharded handle reports the caller's tree index, not its own)
    // (neighbour joining counts matrices, not trees)
    // (placement counts columns and pendant lengths)
    if (st[0] == kBadColumnPattern || st[0] == kBadPendantLength)
      return fail(std::string(status_message(st[0])) + (st[0] == kBadColumnPattern ? " (column " : " (pendant ") +
                  std::to_string(st[1]) + ")");
    // (the split table's capacity: its second word is the number of distinct splits)
    if (st[0] == kSplitCapacity) return fail(std::string(status_message(st[0])) + " (S = " + std::to_string(st[1]) + ")");
    // (the SBN support's capacities: both needed counts)
    if (st[0] == kSbnCapacity)
      return fail(std::string(status_message(st[0])) + " (S = " + std::to_string(st[1]) + ", C = " + std::to_string(st[3]) + ")");
    if (st[0] == kSbnEmptyBlock)
      return fail(std::string(status_message(st[0])) + " (sample " + std::to_string(st[1]) + ", block " + std::to_string(st[3]) + ")");
    if (st[0] == kSbnBadDescent) return fail(std::string(status_message(st[0])) + " (sample " + std::to_string(st[1]) + ")");
    if (st[0] == kBranchModelBadParam)
      return fail(std::string(status_message(st[0])) + " (tree " + std::to_string(st[1] + e->status_tree_offset) +
                  ", edge " + std::to_string(st[3]) + ")");
    if (st[0] == kGpViBadEntry)
      return fail(std::string(status_message(st[0])) + " (tree " + std::to_string(st[1]) + ", node " + std::to_string(st[3]) + ")");
    if (st[0] == kGpTreeBadParam) return fail(std::string(status_message(st[0])) + " (entry " + std::to_string(st[1]) + ")");
    if (st[0] == kGpTreeEmptyBlock)
      return fail(std::string(status_message(st[0])) + " (sample " + std::to_string(st[1]) +
                  (st[3] < 0 ? ", the rootsplits)" : ", block of node " + std::to_string(st[3] >> 1) + ", clade " + std::to_string(st[3] & 1) + ")"));
    if (st[0] == kBootBadWeight) return fail(std::string(status_message(st[0])) + " (pattern " + std::to_string(st[1]) + ")");
    if (st[0] == kBootBadTotal || st[0] == kBootSitesNotTotal) return fail(status_message(st[0]));
    if (st[0] == kSbnBadParam) return fail(std::string(status_message(st[0])) + " (parameter " + std::to_string(st[1]) + ")");
    return fail(std::string(status_message(st[0])) + (st[0] == kBadDistance ? " (matrix " : " (tree ") +
                std::to_string(st[1] + e->status_tree_offset) + ")");
  }
  return 0;
}

const char kShardedDeviceCall[] =
    "device-pointer entry points need a single-device engine: one engine per device (one "
    "process per GPU), or the host-pointer entry points";
const char kHessian4State[] = "the branch-length Hessian call is 4-state only";
const char kNni4State[] = "the NNI neighbourhood scan is 4-state only";
const char kPatternLl4State[] = "per-pattern log-likelihoods are 4-state only";
const char kAncestral4State[] = "the ancestral-state call is 4-state only";
const char kPlacement4State[] = "the placement call is 4-state only";
const char kSpr4State[] = "the SPR neighbourhood scan is 4-state only";

extern "C" {

int32_t mi_abi_version(void) { return MI_PHYLO_ABI_VERSION; }
const char* mi_last_error(void) { return g_error.c_str(); }
int32_t mi_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

int32_t mi_engine_create_device_tips(const mi_engine_spec* spec, const int32_t* device_tip_states,
                                     const double* device_pattern_weights,
                                     mi_engine** out_engine) {
  Switches sw;
  if (read_switches(sw)) return 1;
  if (!device_tip_states || !device_pattern_weights) return fail("null device pointer");
  return create_engine(spec, sw, nullptr, nullptr, {device_tip_states, nullptr, device_pattern_weights, true},
                       out_engine);
}

int32_t mi_engine_create(const mi_engine_spec* spec, const int32_t* tip_states,
                         const double* tip_partials, const double* pattern_weights,
                         mi_engine** out_engine) {
  Switches sw;
  if (read_switches(sw)) return 1;
  return create_engine(spec, sw, nullptr, nullptr, {tip_states, tip_partials, pattern_weights}, out_engine);
}

int32_t mi_engine_create_reversible(const mi_engine_spec* spec, const double* exchangeabilities,
                                    const double* frequencies, const int32_t* tip_states,
                                    const double* tip_partials, const double* pattern_weights,
                                    mi_engine** out_engine) {
  Switches sw;
  if (read_switches(sw)) return 1;
  if (spec && spec->subst_model != MI_SUBST_REVERSIBLE)
    return fail("mi_engine_create_reversible needs subst_model == MI_SUBST_REVERSIBLE");
  if ((exchangeabilities == nullptr) != (frequencies == nullptr))
    return fail("pass both exchangeabilities and frequencies, or neither (built-in WAG)");
  return create_engine(spec, sw, exchangeabilities, frequencies, {tip_states, tip_partials, pattern_weights},
                       out_engine);
}

void mi_engine_destroy(mi_engine* e) {
  if (e) delete e;
}
int64_t mi_device_bytes_held(void) { return miphylo::device_bytes_held.load(); }

int32_t mi_engine_param_count(const mi_engine* e) { return e ? e->param_count : -1; }
int32_t mi_engine_block_count(const mi_engine* e) { return e ? (int32_t)e->blocks.size() : -1; }
int32_t mi_engine_block(const mi_engine* e, int32_t index, const char** name, int32_t* start,
                        int32_t* length) {
  if (!e || index < 0 || index >= (int32_t)e->blocks.size()) return fail("block index out of range");
  if (name) *name = e->blocks[index].name.c_str();
  if (start) *start = e->blocks[index].start;
  if (length) *length = e->blocks[index].length;
  return 0;
}

int32_t mi_engine_reserve(mi_engine* e, int32_t tree_count, int32_t for_gradients) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (!e->shards.empty())
    return for_each_shard(e, tree_count, [&](mi_engine* shard, int c) { return mi_engine_reserve(shard, c, for_gradients); });
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) {
    // a gradient engine may be asked for log-likelihoods too: those calls run more evaluations
    // per launch (fewer vectors each) and size the per-launch operand buffers accordingly
    // A back-off of the arena budget inside either reservation RELEASES every buffer that
    // scales with the budget -- those of the other shape too -- so both are repeated with the
    // reduced budget until a whole pass allocates without backing off: a later *_device call
    // then allocates nothing.  (A back-off also invalidates hipGraphs captured earlier on
    // this engine: their kernels point at released buffers.  include/mi_phylo.h says so.)
    for (int pass = 0; pass < 64; pass++) {
      const int before = e->aa_backoffs;
      if (for_gradients && aa_reserve(e, tree_count, true)) return 1;
      if (aa_reserve(e, tree_count, false)) return 1;
      if (e->aa_backoffs == before) return 0;
    }
    return fail("the partial-vector arena could not be reserved: the budget kept shrinking");
  }
  // Everything a later *_device call over `tree_count` trees can need -- with or without
  // rescaling, whichever optional outputs it asks for --, so that such a call allocates
  // nothing (it can then be captured in a hipGraph): the union of both rescaling settings'
  // plans (the HBM arena when either of them cannot use an on-chip kernel).
  const bool grad = for_gradients != 0;
  if (grad) {  // the fused reductions' per-tree buffers (mi_engine_gradients_unrooted_reduced*)
    if (e->red_ll.ensure(sizeof(double) * tree_count)) return 1;
    if (e->red_g.ensure(sizeof(double) * (size_t)tree_count * e->N)) return 1;
    if (e->red_site.ensure(sizeof(double) * tree_count)) return 1;
  }
  const CallKind kind = grad ? kGradientCall : kLogLikCall;
  return reserve(e, plan_call(e, kind, tree_count, false)) || reserve(e, plan_call(e, kind, tree_count, true));
}

int32_t mi_engine_check_status(mi_engine* e, void* stream) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) {
    for (mi_engine* shard : e->shards) {
      const int rc = check_status(shard, shard->stream);
      shard->fused_timed_out = false;  // (reported to the caller: not a host-pointer call's to repeat)
      if (rc) return 1;
    }
    return 0;
  }
  const int rc = check_status(e, pick_stream(e, stream));
  e->fused_timed_out = false;  // (a device-pointer caller repeats the call itself)
  return rc;
}

static int32_t profile_begin(mi_engine* e, int32_t max_calls, bool phases) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return profile_begin(e->shards[0], max_calls, phases);
  if (max_calls < 0) return fail("max_calls must be >= 0");
  HIP_TRY(hipSetDevice(e->spec.device));
  while ((int)e->prof_events.size() < kProfEvents * max_calls) {
    Event ev;
    HIP_TRY(hipEventCreate(&ev.h));
    e->prof_events.push_back(std::move(ev));
  }
  e->prof_capacity = max_calls;
  e->prof_used = 0;
  e->prof_phases = phases;
  return 0;
}

int32_t mi_engine_profile_begin(mi_engine* e, int32_t max_calls) {
  return profile_begin(e, max_calls, false);
}
int32_t mi_engine_profile_begin_phases(mi_engine* e, int32_t max_calls) {
  return profile_begin(e, max_calls, true);
}

int32_t mi_engine_profile_collect(mi_engine* e, double* out_ms, int32_t capacity,
                                  int32_t* out_count) {
  return mi_engine_profile_collect_phases(e, out_ms, nullptr, capacity, out_count, nullptr);
}

int32_t mi_engine_profile_collect_phases(mi_engine* e, double* out_ms, double* out_phase_ms,
                                         int32_t capacity, int32_t* out_count,
                                         int32_t* out_first_launch_evaluations) {
  if (!e) return fail("null engine");
  if (!e->shards.empty())
    return mi_engine_profile_collect_phases(e->shards[0], out_ms, out_phase_ms, capacity,
                                            out_count, out_first_launch_evaluations);
  if (out_phase_ms && !e->prof_phases)
    return fail("phase times were not recorded: use mi_engine_profile_begin_phases");
  const int count = std::min(e->prof_used, capacity);
  for (int i = 0; i < count; i++) {
    const Event* ev = &e->prof_events[(size_t)kProfEvents * i];
    HIP_TRY(hipEventSynchronize(ev[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (out_ms) out_ms[i] = ms;
    if (out_phase_ms) {
      HIP_TRY(hipEventSynchronize(ev[6]));
      for (int k = 0; k < 4; k++) {
        HIP_TRY(hipEventElapsedTime(&ms, ev[2 + k], ev[3 + k]));
        out_phase_ms[4 * i + k] = ms;
      }
    }
  }
  if (out_count) *out_count = count;
  if (out_first_launch_evaluations) *out_first_launch_evaluations = e->prof_first_launch_evals;
  e->prof_capacity = 0;
  e->prof_used = 0;
  e->prof_phases = false;
  return 0;
}

int32_t mi_engine_last_call_info(const mi_engine* e, const char** dominant_kernel,
                                 int64_t* evaluations, int64_t* gradient_evaluations) {
  if (!e) return fail("null engine");
  if (!e->shards.empty())
    return mi_engine_last_call_info(e->shards[0], dominant_kernel, evaluations,
                                    gradient_evaluations);
  if (dominant_kernel) *dominant_kernel = e->dominant;
  if (evaluations) *evaluations = e->last_evals;
  if (gradient_evaluations) *gradient_evaluations = e->last_grad_evals;
  return 0;
}

const char* mi_engine_last_call_path(const mi_engine* e) {
  if (!e) return "";
  if (!e->shards.empty()) return mi_engine_last_call_path(e->shards[0]);
  return e->last_path.c_str();
}

int32_t mi_engine_last_call_launches(const mi_engine* e, int32_t* walk_launches,
                                     int32_t* arena_backoffs) {
  if (!e) return fail("null engine");
  if (!e->shards.empty())
    return mi_engine_last_call_launches(e->shards[0], walk_launches, arena_backoffs);
  if (walk_launches) *walk_launches = e->last_walk_launches;
  if (arena_backoffs) *arena_backoffs = e->aa_backoffs;
  return 0;
}

/* ---- device-pointer entry points ---------------------------------------- */

int32_t mi_engine_log_likelihoods_unrooted_device(mi_engine* e, void* stream, int32_t T,
                                                  const int32_t* parent_ids, const double* bl,
                                                  const double* params, int32_t rescaling,
                                                  double* out_ll) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  DeviceCall d;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.out_ll = out_ll;
  return run_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_gradients_unrooted_device(mi_engine* e, void* stream, int32_t T,
                                            const int32_t* parent_ids, const double* bl,
                                            const double* params, int32_t rescaling,
                                            double* out_ll, double* out_branch,
                                            double* out_site, double* out_subst) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (!out_branch) return fail("null branch-gradient output");
  DeviceCall d;
  d.gradient = true;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.out_ll = out_ll;
  d.out_branch = out_branch;
  d.out_site = out_site;
  d.out_subst = out_subst;
  return run_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_branch_hessian_unrooted_device(mi_engine* e, void* stream, int32_t T,
                                                 const int32_t* parent_ids, const double* bl,
                                                 const double* params, int32_t rescaling,
                                                 double* out_ll, double* out_branch,
                                                 double* out_hess, double* out_gsq) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kHessian4State);
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (!out_hess) return fail("null branch-Hessian output");
  DeviceCall d;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.out_ll = out_ll;
  d.out_branch = out_branch;
  d.out_hess = out_hess;
  d.out_gsq = out_gsq;
  return run_hessian_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_reserve_hessian(mi_engine* e, int32_t tree_count) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (e->s == kAa) return fail(kHessian4State);
  if (!e->shards.empty()) return for_each_shard(e, tree_count, mi_engine_reserve_hessian);
  HIP_TRY(hipSetDevice(e->spec.device));
  return reserve_hessian_calls(e, tree_count);
}

int32_t mi_engine_nni_scan_unrooted_device(mi_engine* e, void* stream, int32_t T,
                                           const int32_t* parent_ids, const double* bl,
                                           const double* params, int32_t rescaling, double* out_ll,
                                           double* out_delta, int32_t* out_best) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kNni4State);
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (!out_delta) return fail("null NNI delta output");
  DeviceCall d;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.out_ll = out_ll;
  d.out_nni = out_delta;
  d.out_best = out_best;
  return run_nni_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_reserve_nni_scan(mi_engine* e, int32_t tree_count) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (e->s == kAa) return fail(kNni4State);
  if (!e->shards.empty()) return for_each_shard(e, tree_count, mi_engine_reserve_nni_scan);
  HIP_TRY(hipSetDevice(e->spec.device));
  return reserve_nni_calls(e, tree_count);
}

int32_t mi_engine_ancestral_states_unrooted_device(mi_engine* e, void* stream, int32_t T,
                                                   const int32_t* parent_ids, const double* bl,
                                                   const double* params, int32_t rescaling, double* out_ll,
                                                   double* out_state, int8_t* out_map, double* out_cat,
                                                   double* out_rate, double* out_tip) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kAncestral4State);
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (!out_state) return fail("null state-posterior output");
  DeviceCall d;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.out_ll = out_ll;
  d.out_anc_state = out_state;
  d.out_anc_map = out_map;
  d.out_anc_cat = out_cat;
  d.out_anc_rate = out_rate;
  d.out_anc_tip = out_tip;
  return run_ancestral_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_reserve_ancestral(mi_engine* e, int32_t tree_count) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (e->s == kAa) return fail(kAncestral4State);
  if (!e->shards.empty()) return for_each_shard(e, tree_count, mi_engine_reserve_ancestral);
  HIP_TRY(hipSetDevice(e->spec.device));
  return reserve_ancestral_calls(e, tree_count);
}

int32_t mi_engine_placement_unrooted_device(mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                                            const double* bl, const double* params, int32_t rescaling, int32_t Q,
                                            int32_t C, const int8_t* query_states, const int32_t* column_pattern,
                                            const double* column_weights, int32_t G, const double* pendant_lengths,
                                            double* out_ll, double* out_edge_ll, int8_t* out_pendant_index,
                                            int32_t* out_best_edge, double* out_lwr, double* out_edge_tables) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kPlacement4State);
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (check_placement_shape(e, Q, C, G)) return 1;
  if (!query_states || !column_pattern || !pendant_lengths) return fail("null query / column / pendant array");
  if (!out_edge_ll) return fail("null edge log-likelihood output");
  DeviceCall d;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.Q = Q;
  d.C = C;
  d.G = G;
  d.query_states = query_states;
  d.column_pattern = column_pattern;
  d.column_weights = column_weights;
  d.pendant_lengths = pendant_lengths;
  d.out_ll = out_ll;
  d.out_place_edge_ll = out_edge_ll;
  d.out_place_pendant = out_pendant_index;
  d.out_place_best = out_best_edge;
  d.out_place_lwr = out_lwr;
  d.out_place_tables = out_edge_tables;
  return run_placement_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_reserve_placement(mi_engine* e, int32_t tree_count, int32_t query_count, int32_t column_count,
                                    int32_t pendant_count) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (e->s == kAa) return fail(kPlacement4State);
  if (check_placement_shape(e, query_count, column_count, pendant_count)) return 1;
  if (!e->shards.empty()) {
    if (e->shard_mode != MI_SHARD_TREES) return fail("pattern-sharded engines do not place queries");
    return for_each_shard(e, tree_count, [=](mi_engine* shard, int32_t count) {
      return mi_engine_reserve_placement(shard, count, query_count, column_count, pendant_count);
    });
  }
  HIP_TRY(hipSetDevice(e->spec.device));
  return reserve_placement_calls(e, tree_count, pendant_count);
}

int32_t mi_engine_spr_scan_unrooted_device(mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                                           const double* bl, const double* params, int32_t rescaling,
                                           int32_t radius, double* out_ll, int32_t* out_best_target,
                                           double* out_best_delta, int32_t* out_best_move, double* out_delta) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kSpr4State);
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (check_spr_shape(e, radius)) return 1;
  if (!out_best_target || !out_best_delta) return fail("null best-target / best-delta output");
  DeviceCall d;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.spr_radius = radius;
  d.out_ll = out_ll;
  d.out_spr_target = out_best_target;
  d.out_spr_delta = out_best_delta;
  d.out_spr_move = out_best_move;
  d.out_spr_table = out_delta;
  return run_spr_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_reserve_spr_scan(mi_engine* e, int32_t tree_count) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (e->s == kAa) return fail(kSpr4State);
  if (!e->shards.empty()) {
    if (e->shard_mode != MI_SHARD_TREES) return fail("pattern-sharded engines do not scan SPR neighbourhoods");
    return for_each_shard(e, tree_count, mi_engine_reserve_spr_scan);
  }
  if (check_spr_shape(e, 0)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  return reserve_spr_calls(e, tree_count);
}

int32_t mi_engine_log_likelihoods_rooted_device(mi_engine* e, void* stream, int32_t T,
                                                const int32_t* parent_ids, const double* bl,
                                                const double* params, const double* rates,
                                                const double* heights, const double* bounds,
                                                int32_t with_jacobian, int32_t rescaling,
                                                double* out_ll) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (with_jacobian && (!rates || !heights || !bounds))
    return fail("Attempted access of a time tree member that requires the time tree to be "
                "initialized. Have you set dates for your time trees, and initialized the "
                "time trees?");
  DeviceCall d;
  d.rooted = true;
  d.with_jacobian = with_jacobian != 0;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.rates = rates;
  d.heights = heights;
  d.bounds = bounds;
  d.out_ll = out_ll;
  return run_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_gradients_rooted_device(mi_engine* e, void* stream, int32_t T,
                                          const int32_t* parent_ids, const double* bl,
                                          const double* params, const double* rates,
                                          const int32_t* rate_counts, const double* heights,
                                          const double* bounds, const double* ratios,
                                          int32_t rescaling, double* out_ll, double* out_ratios,
                                          double* out_clock, double* out_site,
                                          double* out_subst) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (!rates || !rate_counts || !heights || !bounds || !ratios)
    return fail("Attempted access of a time tree member that requires the time tree to be "
                "initialized. Have you set dates for your time trees, and initialized the "
                "time trees?");
  if (!out_ratios || !out_clock) return fail("null gradient output");
  DeviceCall d;
  d.gradient = true;
  d.rooted = true;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.rates = rates;
  d.rate_counts = rate_counts;
  d.heights = heights;
  d.bounds = bounds;
  d.ratios = ratios;
  d.out_ll = out_ll;
  d.out_ratios = out_ratios;
  d.out_clock = out_clock;
  d.out_site = out_site;
  d.out_subst = out_subst;
  return run_device(e, pick_stream(e, stream), d);
}

// rocPRIM is asked for its temporary-storage size once per (entries, key bits), not per call
static size_t reduce_workspace_bytes(mi_engine* e, int32_t T, int32_t index_count) {
  const long entries = (long)T * e->N;
  int bits = 1;
  while (bits < 32 && (1u << bits) <= (uint32_t)index_count) bits++;
  if (e->red_ws_entries != entries || e->red_ws_bits != bits) {
    e->red_ws_bytes = vi_reduce_workspace_bytes(entries, index_count);
    e->red_ws_entries = entries;
    e->red_ws_bits = bits;
  }
  return e->red_ws_bytes;
}

int32_t mi_engine_reserve_reduced(mi_engine* e, int32_t tree_count, int32_t index_count) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return mi_engine_reserve(e, tree_count, 1);  // (host-pointer calls only)
  if (index_count < 0) return fail("index_count must be >= 0");
  if (mi_engine_reserve(e, tree_count, 1)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if ((uint64_t)tree_count * (uint64_t)e->N > 0xffffffffull)
    return fail("the fused reductions number their (tree, node) entries in 32 bits: tree_count x "
                "(2 taxa - 1) must stay below 2^32");
  return e->red_sort.ensure(reduce_workspace_bytes(e, tree_count, index_count));
}

/* Engine::Gradients followed by the caller-side reductions of one variational-inference
 * step (vip/burrito.py:143-166, vip/branch_model.py:104-133,
 * src/unrooted_sbn_instance.cpp:176-198), fused behind the call: see include/mi_phylo.h. */
int32_t mi_engine_gradients_unrooted_reduced_device(
    mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids, const double* bl,
    const double* params, int32_t rescaling, const int32_t* branch_index,
    const double* tree_weights, int32_t index_count, double* out_sums,
    double* out_index_gradient, double* out_ll) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (!branch_index || !out_sums || index_count < 0 || (index_count > 0 && !out_index_gradient))
    return fail("null output / index");
  hipStream_t s = pick_stream(e, stream);
  HIP_TRY(hipSetDevice(e->spec.device));
  // per-tree results into the engine's own buffers unless the caller wants logL too
  if (e->red_ll.ensure(sizeof(double) * std::max(T, 1))) return 1;
  if (e->red_g.ensure(sizeof(double) * (size_t)std::max(T, 1) * e->N)) return 1;
  if (e->red_site.ensure(sizeof(double) * std::max(T, 1))) return 1;
  double* ll = out_ll ? out_ll : e->red_ll.as<double>();
  DeviceCall d;
  d.gradient = true;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.out_ll = ll;
  d.out_branch = e->red_g.as<double>();
  d.out_site = e->K > 1 ? e->red_site.as<double>() : nullptr;
  d.out_subst = nullptr;  // (the 16 finite-difference passes are not part of this reduction)
  if (run_device(e, s, d)) return 1;
  ViReduceArgs ra{};
  ra.T = T;
  ra.N = e->N;
  ra.index_count = index_count;
  ra.ll = ll;
  ra.branch = e->red_g.as<double>();
  ra.site = e->K > 1 ? e->red_site.as<double>() : nullptr;
  ra.branch_index = branch_index;
  ra.tree_weights = tree_weights;
  ra.out_sums = out_sums;
  ra.out_index_gradient = out_index_gradient;
  if ((uint64_t)T * (uint64_t)e->N > 0xffffffffull)
    return fail("the fused reductions number their (tree, node) entries in 32 bits: tree_count x "
                "(2 taxa - 1) must stay below 2^32");
  const size_t ws = reduce_workspace_bytes(e, T, index_count);
  if (e->red_sort.ensure(ws)) return 1;
  if (launch_vi_reduce(ra, e->red_sort.ptr, ws, s)) return fail("the index sort of the reduction could not be launched");
  HIP_TRY(hipGetLastError());
  return 0;
}

int32_t mi_engine_create_sharded(const mi_engine_spec* spec, int32_t shard_count,
                                 const int32_t* devices, int32_t shard_mode,
                                 const double* exchangeabilities, const double* frequencies,
                                 const int32_t* tip_states, const double* tip_partials,
                                 const double* pattern_weights, mi_engine** out_engine) {
  Switches sw;  // (one snapshot for every shard)
  if (read_switches(sw)) return 1;
  if (!spec || !out_engine) return fail("null spec / out_engine");
  *out_engine = nullptr;
  if (shard_count <= 0) return fail("Thread count needs to be strictly positive.");  // engine.cpp:14-16
  if (shard_mode != MI_SHARD_TREES && shard_mode != MI_SHARD_PATTERNS)
    return fail("unknown shard mode");
  if (shard_mode == MI_SHARD_PATTERNS && shard_count > spec->pattern_count)
    return fail("more pattern shards than site patterns");
  const int count = mi_device_count();
  if (count == 0) return fail("no HIP device available: the MI355X engine has no CPU fallback");
  int current = 0;
  if (hipGetDevice(&current) != hipSuccess) current = 0;
  std::unique_ptr<mi_engine> front(new mi_engine());
  front->spec = *spec;
  front->sw = sw;
  front->shard_mode = shard_mode;
  front->n = spec->taxon_count;
  front->N = 2 * front->n - 1;
  front->P = spec->pattern_count;
  front->K = spec->category_count;
  const int n = spec->taxon_count, P = spec->pattern_count;
  for (int i = 0; i < shard_count; i++) {
    mi_engine_spec sub = *spec;
    // NULL: round-robin over the visible devices STARTING AT THE CALLER'S CURRENT DEVICE (a
    // one-process-per-GPU launch that selected its device with hipSetDevice keeps it; a
    // negative ordinal -1 - k names "the k-th device from the current one" explicitly)
    int want = devices ? devices[i] : -1 - i;
    if (want < 0) want = (current + (-1 - want)) % count;
    sub.device = want;
    TipSource tips{tip_states, tip_partials, pattern_weights};
    std::vector<int32_t> states;
    std::vector<double> partials;
    if (shard_mode == MI_SHARD_PATTERNS) {
      int32_t b = 0, c = P;
      mi_shard_range(P, shard_count, i, &b, &c);
      sub.pattern_count = c;
      tips = {slice_columns(tip_states, n, P, b, c, 1, states),
              slice_columns(tip_partials, n, P, b, c, spec->state_count, partials), pattern_weights + b};
    }
    mi_engine* shard = nullptr;
    if (create_engine(&sub, sw, exchangeabilities, frequencies, tips, &shard)) return 1;
    front->shards.push_back(shard);
  }
  const mi_engine* first = front->shards[0];
  front->param_count = first->param_count;
  front->blocks = first->blocks;
  front->s = first->s;
  *out_engine = front.release();
  return 0;
}

int32_t mi_engine_shard_count(const mi_engine* e) {
  return e ? std::max<int32_t>(1, (int32_t)e->shards.size()) : -1;
}

int32_t mi_engine_shard_device(const mi_engine* e, int32_t shard) {
  if (!e) return -1;
  if (e->shards.empty()) return shard == 0 ? e->spec.device : -1;
  if (shard < 0 || shard >= (int32_t)e->shards.size()) return -1;
  return e->shards[shard]->spec.device;
}


}  // extern "C"
