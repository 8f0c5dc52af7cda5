// The 4-state call: which route a call takes (plan_call), what it reserves, its argument
// blocks and its launch sequence.  Compiled with hipcc; no torch.
//
// Per call (all on one HIP stream, no host synchronisation in the *_device path):
//   tree_setup -> model_setup -> transition -> {loglik_* | gradient_walk* | gradient_hbm}*
//   -> reduce_tiles -> finalize
#include "mi_phylo_engine.h"

namespace {

// (waves: one-wave workgroups of a gradient launch; default: a large batch)
bool use_arena(const mi_engine* e, bool rescale, bool subst, size_t waves = (size_t)-1, int regs = 0) {
  // (the look-up walk's arena variant starts one step earlier: gradient_walk_use_arena)
  const bool lut = walk3_possible(e) && e->sw.walk3_arena && !subst && gradient_mfma_groups(e->K) == 1;
  return gradient_walk_use_arena(e->sw.gradient_store, e->n, e->K, rescale, subst, waves, lut, regs);
}
bool walk_fits(const mi_engine* e, bool rescale) { return gradient_walk_fits(e->n, e->K, rescale); }

// which log-likelihood kernel a call uses (also decides who fills the tip tables)
const char* loglik_kernel_of(const mi_engine* e, bool rescaling) {
  LikArgs probe{};
  probe.n = e->n;
  probe.K = e->K;
  probe.tip_masks = e->have_tip_masks ? e->tip_masks.as<uint8_t>() : nullptr;
  return loglik_kernel_name(probe, rescaling, e->max_slots, e->sw);
}
// Does a gradient call run on the matrix-core walk kernel?  (K > 4: the kernel takes the site
// likelihoods from a pass of the matrix-core log-likelihood kernel; if that one cannot run,
// neither can it.)
bool matrix_core_gradient(const mi_engine* e, bool rescaling, bool loglik_is_valu) {
  return !e->sw.hbm_gradient && e->have_tip_masks && walk_fits(e, rescaling) &&
         reduce_tiles_fits(e->N) && (gradient_mfma_groups(e->K) == 1 || !loglik_is_valu);
}

size_t plv_bytes_per_eval(const mi_engine* e) {
  return (size_t)(e->n - 1) * e->K * e->tiles * kTile * 4 * sizeof(double);
}
// HBM one evaluation of the call's gradient / Hessian kernel needs while it runs (0: none)
size_t vector_bytes_per_eval(const mi_engine* e, const CallPlan& p) {
  return !p.mfma ? plv_bytes_per_eval(e)
                 : p.store == kStoreArena ? gradient_arena_bytes_per_eval(e->n, e->P, e->K) : 0;
}

// one launch covers at most kMaxEvals evaluations (grid y dimension: 65535; a multiple
// of 8 keeps whole evaluations per XCD)
constexpr int kMaxEvals = 32768;
// launch(first, count) over `count` evaluations in parts of at most min(kMaxEvals, what the
// vector arena `plv` holds at bytes_per_eval each; 0: no arena in use); returns the first part's size
template <typename F>
int launch_in_parts(const mi_engine* e, int count, size_t bytes_per_eval, int& walk_launches, F launch) {
  const int part = bytes_per_eval
                       ? (int)std::max<size_t>(1, std::min<size_t>(kMaxEvals, e->plv.bytes / bytes_per_eval))
                       : kMaxEvals;
  for (int done = 0; done < count; done += part) {
    walk_launches++;
    launch(done, std::min(part, count - done));
  }
  return std::min(part, count);
}

const MacroEntry* walk_macros(const mi_engine* e, const CallPlan& p) {
  return p.store == kStoreArena ? e->arena_macros.as<MacroEntry>() : e->macros.as<MacroEntry>();
}

}  // namespace

// Can calls of this engine take the third-generation walk (kernels_walk3.hip)?  (Per call it
// also needs no analytic substitution gradient.)  Which generation of the matrix-core gradient
// walk a call takes: the third (kernels_walk3.hip: tip children looked up; one-hot / all-ones
// tips, at most four rate categories, no analytic substitution gradient -- everything the
// reference produces) wherever it applies, else the second (kernels_walk.hip: mask tips, any
// category count, analytic gradient).  MI_PHYLO_GRADIENT_WALK=v2 keeps every call on the second.
// (The first generation, gradient_mfma_kernel, was retired in round 6: the second had been ahead
// of it on every shape but the arena shapes with fewer than three categories and a handful of
// tiles -- fluA: 0.321 against 0.335 ms per 1000 trees -- and those now take the third: 0.305 ->
// 0.29.)
bool walk3_possible(const mi_engine* e) {
  return e->sw.walk3 && e->have_tip_codes && gradient_walk_lut_applies(e->K);
}

// The look-up walk's tile width for this engine (kernels_walk3.hip, RR; gradient_walk_tile_regs):
// wide tiles pay in the arena variant, so an engine gets them if its batches take the arena --
// and then for every look-up-walk call: sums over patterns are formed tile by tile, and a
// tree's outputs must not depend on the size of the batch it came in.  (Its calls of a few
// trees keep every vector in LDS with the same wide tiles, one wave per SIMD:
// gradient_walk_use_arena.)
int engine_tile_regs(const mi_engine* e) {
  const bool lut = walk3_possible(e) && e->sw.walk3_arena && gradient_mfma_groups(e->K) == 1;
  const int forced = e->sw.walk_tile_regs;
  const int r = lut && (forced || gradient_walk_batches_take_arena(e->n, e->K, true)) ? gradient_walk_tile_regs(e->n, e->P, e->K, forced) : 0;
  return r > kLlR ? r : 0;
}

CallPlan plan_call(const mi_engine* e, CallKind kind, int T, bool rescaling, int route_T, bool rooted,
                   bool want_site, bool want_subst) {
  CallPlan p{};
  const int n = e->n;
  const bool gradient = kind == kGradientCall;
  p.kind = kind;
  p.T = T;
  p.rescaling = rescaling;
  p.rooted = rooted;
  p.gtr = e->spec.subst_model == MI_SUBST_GTR;
  p.groups = 1;
  p.models_per_tree = 1;
  p.E = p.M = T;
  p.mmats_bytes_per_eval = std::max(gradient_walk_mats_bytes_per_eval(n, e->K),
                                    walk3_possible(e) ? gradient_walk_lut_mats_bytes_per_eval(n) : 0);
  // which log-likelihood kernel runs (also decides who fills the tip tables, below)
  p.dominant = loglik_kernel_of(e, rescaling);
  p.loglik_is_valu = std::string(p.dominant) == "loglik_onchip_kernel";
  if (kind == kHessianCall) {
    // The branch-length Hessian call: one evaluation per tree with the tree's own
    // model, as the `light` GTR call.  Either the Hessian form of the second-generation
    // matrix-core walk (K <= 4, tip masks, the tree fits the walk) or the Hessian form of the
    // HBM-streamed gradient kernel (everything else, and MI_PHYLO_GRADIENT_PATH=hbm).
    p.Eg = T;
    p.mfma = !e->sw.hbm_gradient && e->have_tip_masks && e->K <= 4 && walk_fits(e, rescaling);
    p.g_tiles = p.mfma ? gradient_mfma_tiles(e->P, e->K) : e->tiles;
    // the walk form's store: the plain walk's rule for a batch of this many waves (one per tile)
    const size_t waves = (size_t)(route_T ? route_T : T) * gradient_mfma_tiles(e->P, e->K);
    const bool arena = p.mfma && gradient_walk_use_arena(e->sw.gradient_store, n, e->K, rescaling, false, waves, false, 0);
    p.store = !p.mfma ? kStoreHbm : arena ? kStoreArena : kStoreLds;
    p.reserve_arena = arena;
    p.need_slots = !p.mfma;  // (the HBM kernel walks the node-level schedule)
    p.dominant = p.mfma ? gradient_walk_hess_kernel_name() : gradient_hessian_kernel_name();
    return p;
  }
  if (kind == kNniCall) {
    // The NNI neighbourhood scan: one evaluation per tree with the tree's own
    // model; always the node-ordered matrices and the HBM-streamed kernel (which finds its way
    // in a schedule of any order: no LDS slots asked for).
    p.Eg = T;
    p.g_tiles = e->tiles;
    p.store = kStoreHbm;
    p.dominant = nni_scan_kernel_name();
    return p;
  }
  if (kind == kAncestralCall) {
    // Ancestral-state and rate-category posteriors: as the scan -- one evaluation
    // per tree with the tree's own model, node-ordered matrices, the HBM-streamed kernel.
    p.Eg = T;
    p.g_tiles = e->tiles;
    p.store = kStoreHbm;
    p.dominant = ancestral_kernel_name();
    return p;
  }
  if (kind == kPlacementCall) {
    // Placement: as the ancestral-state call -- one evaluation per tree with the
    // tree's own model, node-ordered matrices, the HBM-streamed kernel.
    p.Eg = T;
    p.g_tiles = e->tiles;
    p.store = kStoreHbm;
    p.dominant = placement_kernel_name();
    return p;
  }
  if (kind == kSprCall) {
    // The SPR neighbourhood scan: as the NNI scan -- one evaluation per tree with
    // the tree's own model, node-ordered matrices, the HBM-streamed kernel.
    p.Eg = T;
    p.g_tiles = e->tiles;
    p.store = kStoreHbm;
    p.dominant = spr_kernel_name();
    return p;
  }
  // on-chip gradient kernels: the matrix-core one (K <= 4; rescaling supported) or the
  // VALU one (no rescaling); everything else takes the HBM-streamed kernel
  p.mfma = gradient && matrix_core_gradient(e, rescaling, p.loglik_is_valu);
  if (p.mfma) p.groups = gradient_mfma_groups(e->K);
  p.analytic = e->sw.analytic_subst && p.mfma && p.gtr;
  // (a wide-tile engine: every call the look-up walk can take runs it, with wide tiles)
  p.tile_regs = p.mfma && !p.analytic && p.groups == 1 ? e->tile_regs : 0;
  p.g_tiles = p.mfma ? gradient_mfma_tiles(e->P, e->K, p.tile_regs) * p.groups : e->tiles;
  // A GTR gradient call whose caller wants neither the substitution-model nor the site-model
  // gradient (BASELINE configs[2] as worded: log-likelihood + branch-length gradient) is ONE
  // evaluation per tree with the tree's own model, exactly like a JC69 call: no perturbed
  // model instances, no finite-difference passes -- and it can take the one-launch path.
  // What it delivers is bit-identical to the full call's.
  p.light = gradient && p.mfma && !p.analytic && p.gtr && !want_subst && !want_site;
  // The evaluation shape.  analytic: the opt-in analytic substitution gradient replaces the 16
  // finite-difference evaluations (and with them the perturbed-model site pass): one gradient
  // evaluation per tree, as for JC69.  (also for the `light` call: the finite-difference passes
  // and the perturbed-model site pass would be computed for nobody)
  const bool fd = gradient && p.gtr && !p.analytic && !p.light;
  p.site_fused = gradient && e->K > 1 && !fd;
  p.site_separate = gradient && e->K > 1 && fd;
  p.models_per_tree = fd ? kFdModels : 1;
  p.M = T * p.models_per_tree;
  p.Eg = gradient ? T : 0;
  if (fd) p.E += 16 * T;
  if (p.site_separate) {
    p.E += T;
    p.Eg += T;
  }
  // the Sethi-Ullman schedule with LDS slots is what the log-likelihood kernels walk
  p.need_slots = !(gradient && p.mfma && p.groups == 1 && (!p.gtr || p.analytic || p.light));
  // (a call of a few trees keeps its stored vectors in LDS however large the tree)
  const bool arena = p.mfma && use_arena(e, rescaling, p.analytic, (size_t)T * (size_t)p.g_tiles, p.tile_regs);
  p.store = !p.mfma ? kStoreHbm : arena ? kStoreArena : kStoreLds;
  // (reservation: the arena variant of the matrix-core kernel keeps its stored vectors in the HBM
  // kernel's buffer -- kept for whichever rescaling setting, batch size or substitution-gradient
  // form of this engine takes it)
  p.reserve_arena = p.mfma && (e->tile_regs || use_arena(e, false, true) || use_arena(e, true, true) ||
                               use_arena(e, false, false) || use_arena(e, true, false));
  // hand-off words of the one-launch small call: kept by every engine whose calls may take it
  p.hand_off_words = gradient && e->fused_setup && walk3_possible(e);
  // The one-launch call (kernels_walk3.hip): tree set-up, model instances and operand records
  // ride in the walk's launch.  One evaluation and one model instance per tree (JC69-type
  // calls), trees of at most 64 nodes, one walk launch, nobody else reads the schedule's LDS
  // slots.  (MI_PHYLO_FUSE_FINALIZE=0: neither this nor the fused reduction, below.)
  // Up to 512 trees: the set-up waves take wave slots the walk would use (four waves of ~10
  // microseconds per tree, a GTR eigensystem on one lane of each) -- measured, DS1
  // (tools/bench_fused_scan.py): one launch / four launches 0.91 at 1-8 trees,
  // 0.98 at 250-500, 0.99 at 1000 (JC69; GTR 1.00), 1.01 beyond.  MI_PHYLO_FUSED_MAX_TREES
  // moves the cross-over (testing).  (The hand-off words exist: reserve, p.hand_off_words.)
  const bool fuse_possible = p.mfma && walk3_possible(e) && !p.analytic && p.groups == 1 && !arena && !p.tile_regs && e->fused_setup &&
                             e->sw.fuse_finalize && p.E == T && p.models_per_tree == 1 && !p.need_slots &&
                             T <= e->sw.fused_max_trees && gradient_walk_lut_fused_applies(n, e->K);
  // The third-generation (look-up) walk: stored vectors in LDS or, since round 6, in the arena.
  // One rate category with the stored vectors in LDS.  The second generation, whose waves take
  // several tiles of a tree in a row, was 5-7 % ahead on a large batch (DS1 x 1000 with the
  // constant site model 0.281 against 0.297 ms) and the look-up walk, with its one-launch call,
  // 6-20 % ahead up to 500 trees (profiles/r06_k1_small_batches.txt): so the rule was "look-up
  // walk where the one-launch call applies".  With the tip codes pre-tiled (a one-category wave
  // regrouped 16 columns of fields per tip: a quarter of its vector instructions) the look-up
  // walk is level on large batches too -- 1000 / 4000 trees, second generation / look-up walk:
  // DS1's shape 0.282 / 0.281 and 0.970 / 0.976 ms, 31 x 1000 0.360 / 0.365 and 1.26 / 1.31, 16 x
  // 500 0.112 / 0.106 and 0.373 / 0.364, 29 x 1195 0.362 / 0.361 and 1.39 / 1.28
  // (profiles/r06_k1_large_batches.txt) -- and takes every one-category call
  // (MI_PHYLO_WALK3_K1=0: the old rule).  (Two and three categories: look-up walk 0.462 / 0.490
  // and 0.831 / 0.868 ms per 1000 DS1 trees.)
  p.walk3 = p.mfma && walk3_possible(e) && !p.analytic && p.groups == 1 &&
            (p.tile_regs || (arena ? e->sw.walk3_arena : (e->K > 1 || e->sw.walk3_k1_lds || fuse_possible)));
  p.fuse_setup = p.walk3 && fuse_possible;
  // Beyond the one-launch call's size the same set-up waves CAN run as one launch in front of the
  // walk's (round 6, MI_PHYLO_SETUP_RECORDS=1): trees, model instances and operand records --
  // instead of the tree set-up launch and the record launch, 13 + 18 us of a 1000-tree DS1 step.
  // Built, bit-identical (test), and not the default: the four quarter-waves of a tree each build
  // the tree, and 4 000 of them take what the two launches take -- the replayed headline step
  // 0.7826 against 0.7823 ms (tools/ab_kernels.py, four rounds), direct launches -1 %.
  const bool records_possible = p.walk3 && !p.fuse_setup && !arena && !p.tile_regs && !p.analytic && p.groups == 1 &&
                                e->fused_setup && p.E == T && p.models_per_tree == 1 && !p.need_slots && T <= kMaxEvals &&
                                gradient_walk_lut_fused_applies(n, e->K);
  p.setup_records = records_possible && e->sw.setup_records == 1;
  // The same in a four-wave workgroup per tree (launch_setup_workgroups): the tree and the model
  // instance are built once, side by side, and all of a 1000-tree batch's workgroups are resident
  // at once.  Taken where a tree has more rows of records than one wave has lanes -- below that,
  // four waves per tree are three idle ones -- (MI_PHYLO_SETUP_RECORDS=wg: wherever it can be;
  // =0, MI_PHYLO_FUSE_FINALIZE=0: the two launches).  DESIGN.md 4.7.
  p.setup_wg = records_possible && (e->sw.setup_records == 2 ||
                                    (e->sw.setup_records < 0 && e->sw.fuse_finalize && (e->N - 1) * e->K > 64));
  // The C ABI's outputs are optional, and work nobody reads is not done: without a
  // substitution-gradient output the 16 finite-difference log-likelihood passes of a GTR
  // call are skipped, without a site-gradient output the extra gradient pass under the
  // perturbed model (section 8 of DESIGN.md) too.  The evaluations keep their numbers; what
  // is delivered is bit-identical to the full call.
  p.fd_pass = gradient && p.gtr && !p.analytic && want_subst;
  p.site_pass = p.site_separate && want_site;
  p.loglik_runs = !gradient || p.fd_pass || (p.mfma && p.groups > 1);
  // the per-state tip tables feed the VALU walk kernels only
  // (only the VALU log-likelihood kernel reads them)
  p.need_tip_tables = p.loglik_runs && p.loglik_is_valu;
  if (gradient)
    p.dominant = p.fuse_setup ? gradient_walk_lut_fused_kernel_name()
                 : p.walk3    ? gradient_walk_lut_kernel_name()
                 : p.mfma     ? gradient_walk_kernel_name()
                              : gradient_kernel_name();
  return p;
}

// which path the call took, for diagnostics (mi_engine_last_call_path)
std::string plan_path(const mi_engine* e, const CallPlan& p) {
  std::string path = p.dominant;
  if (p.kind != kLogLikCall)
    path += p.store == kStoreHbm ? " store=hbm" : (p.store == kStoreArena ? " store=arena" : " store=lds");
  path += p.fuse_setup      ? " setup=in-walk"
          : p.setup_records ? " setup=with-records"
          : p.setup_wg      ? " setup=workgroup-records"
                            : " setup=own-launch";
  if (p.kind == kHessianCall) path += " hess";
  if (p.kind == kNniCall) path += " nni";
  if (p.kind == kAncestralCall) path += " ancestral";
  if (p.kind == kPlacementCall) path += " placement";
  if (p.kind == kSprCall) path += " spr";
  if (p.pattern_ll) path += " pattern_ll";
  if (p.tile_regs > kLlR) path += " tile=wide";
  if (p.fd_pass) path += " fd=16";
  if (p.site_pass) path += " site-pass";
  if (p.light) path += " light";
  if (p.analytic) path += " analytic";
  if (p.rescaling) path += " rescaled";
  if (p.rooted) path += " rooted";
  return path + " K=" + std::to_string(e->K);
}

// Everything the planned call needs, so that it allocates nothing (mi_engine_reserve: it can
// then be captured in a hipGraph).
int reserve(mi_engine* e, const CallPlan& p) {
  const int n = e->n, N = e->N, T = p.T;
  const bool gradient = p.kind == kGradientCall;
  if (e->tree_scratch.ensure(sizeof(int32_t) * (size_t)T * 13 * N)) return 1;
  if (e->sched.ensure(sizeof(SchedEntry) * (size_t)T * (n - 1))) return 1;
  if (e->macros.ensure(sizeof(MacroEntry) * (size_t)T * macro_stride(n))) return 1;
  if (e->macro_count.ensure(sizeof(int32_t) * (size_t)T)) return 1;
  if (e->bl_eff.ensure(sizeof(double) * (size_t)T * N)) return 1;
  if (e->models.ensure(sizeof(DevModel) * (size_t)p.M)) return 1;
  if (e->mats.ensure(sizeof(double) * (size_t)p.E * (N - 1) * e->K * 16)) return 1;
  if (e->tip_tables.ensure(sizeof(double) * (size_t)p.E * n * e->K * 20)) return 1;
  if (gradient) {
    // matrices in the walk's order, per gradient evaluation (kernels_walk.hip)
    if (e->mmats.ensure(p.mmats_bytes_per_eval * (size_t)p.Eg)) return 1;
    if (p.analytic && e->mphi.ensure(p.mmats_bytes_per_eval / 2 * (size_t)p.Eg)) return 1;
  }
  if (p.analytic && e->x_sum.ensure(sizeof(double) * (size_t)p.Eg * kSubstExtra)) return 1;
  if (e->ll_part.ensure(sizeof(double) * (size_t)p.E * e->ll_stride)) return 1;
  if (e->fin_scratch.ensure(sizeof(double) * (size_t)T * 6 * n)) return 1;
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  if (p.hand_off_words && e->ready.bytes < sizeof(int32_t) * kReadyStride * (size_t)T) {
    // hand-off words of the one-launch small call: zero whenever no such call is running
    if (e->ready.ensure(sizeof(int32_t) * kReadyStride * (size_t)T)) return 1;
    HIP_TRY(hipMemset(e->ready.ptr, 0, e->ready.bytes));
    HIP_TRY(hipDeviceSynchronize());
  }
  if (e->ll_sum.ensure(sizeof(double) * (size_t)p.E)) return 1;
  // (the per-pattern call's log-likelihoods when its caller wants none)
  if (p.kind == kLogLikCall && !p.rooted && e->pattern_ll_out.ensure(sizeof(double) * (size_t)T)) return 1;
  if (gradient && e->g_sum.ensure(sizeof(double) * (size_t)p.Eg * 2 * N)) return 1;
  if (gradient) {
    // the HBM-streamed kernel is the fallback for rescaling / trees that do not fit
    // in LDS; its arena is only allocated when that path is taken
    const size_t per = plv_bytes_per_eval(e);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(p.Eg, e->plv_budget / per));
    if (!p.mfma && e->plv.ensure(per * chunk)) return 1;
    // the arena variant of the matrix-core kernel keeps its stored vectors in the same buffer
    if (p.reserve_arena) {
      const size_t aper = gradient_arena_bytes_per_eval(n, e->P, e->K);
      const size_t achunk = std::max<size_t>(1, std::min<size_t>(p.Eg, e->plv_budget / aper));
      if (e->plv.ensure(aper * achunk)) return 1;
      if (e->arena_macros.ensure(sizeof(MacroEntry) * (size_t)T * macro_stride(n))) return 1;
      if (e->slot_need.ensure(sizeof(int32_t) * (size_t)T)) return 1;
    }
    const size_t g_width = std::max<size_t>(2 * (size_t)N, (size_t)gradient_mfma_width(n, true));
    if (e->g_part.ensure(sizeof(double) * (size_t)p.Eg * e->ll_stride * gradient_mfma_groups(e->K) *
                         g_width))
      return 1;
    if (e->site_lik.ensure(sizeof(double) * (size_t)p.Eg * e->tiles * kTile)) return 1;
    if (e->site_exp.ensure(sizeof(int32_t) * (size_t)p.Eg * e->tiles * kTile)) return 1;
  }
  return 0;
}

// ---- one builder per argument block: the engine's buffers, the call's pointers, the plan ----

TreeSetupArgs tree_setup_args(const mi_engine* e, const DeviceCall& d, const CallPlan& p) {
  TreeSetupArgs ts{};
  ts.n = e->n;
  ts.T = d.T;
  ts.rooted = d.rooted;
  ts.parent_ids = d.parent_ids;
  ts.bl = d.bl;
  // rooted trees: LogLikelihood/Gradient scale by rates (fat_beagle.cpp:96-101,507-511);
  // UnrootedLogLikelihood(RootedTree) does not (:78-80).
  ts.rates = (d.rooted && (d.gradient || d.with_jacobian)) ? d.rates : nullptr;
  ts.scratch = e->tree_scratch.as<int32_t>();
  ts.sched = e->sched.as<SchedEntry>();
  // (the gradient schedule is only built for gradient calls that walk it)
  ts.macros = p.mfma ? e->macros.as<MacroEntry>() : nullptr;
  ts.macro_count = e->macro_count.as<int32_t>();
  ts.bl_eff = e->bl_eff.as<double>();
  ts.status = e->status.as<int32_t>();
  ts.max_slots = e->max_slots;
  ts.need_slots = p.need_slots;
  // (arena calls: the slot assignment rides in the set-up launch where a workgroup builds the tree)
  ts.arena_macros = p.store == kStoreArena ? e->arena_macros.as<MacroEntry>() : nullptr;
  ts.slot_need = e->slot_need.as<int32_t>();
  return ts;
}

ModelSetupArgs model_setup_args(const mi_engine* e, const DeviceCall& d, const CallPlan& p) {
  ModelSetupArgs ms{};
  ms.T = d.T;
  ms.models_per_tree = p.models_per_tree;
  ms.subst = e->spec.subst_model;
  ms.site = e->spec.site_model;
  ms.K = e->K;
  ms.param_count = e->param_count;
  ms.rates_off = e->rates_off;
  ms.freqs_off = e->freqs_off;
  ms.shape_off = e->shape_off;
  ms.params = d.params;
  ms.models = e->models.as<DevModel>();
  ms.status = e->status.as<int32_t>();
  ms.weibull_x = e->weibull_x.as<double>();
  return ms;
}

FinalizeArgs finalize_args(const mi_engine* e, const DeviceCall& d) {
  FinalizeArgs fa{};
  fa.n = e->n;
  fa.N = e->N;
  fa.T = d.T;
  fa.K = e->K;
  fa.tiles = e->tiles;
  fa.gradient = d.gradient;
  fa.rooted = d.rooted;
  fa.with_jacobian = d.with_jacobian;
  fa.bl_eff = e->bl_eff.as<double>();
  fa.bl_raw = d.bl;
  fa.rates = d.rates;
  fa.rate_counts = d.rate_counts;
  fa.node_heights = d.heights;
  fa.node_bounds = d.bounds;
  fa.height_ratios = d.ratios;
  fa.sched = e->sched.as<SchedEntry>();
  fa.scratch = e->fin_scratch.as<double>();
  fa.out_ll = d.out_ll;
  fa.out_branch = d.out_branch;
  fa.out_ratios = d.out_ratios;
  fa.out_clock = d.out_clock;
  fa.out_site = d.out_site;
  fa.status = e->status.as<int32_t>();
  return fa;
}

namespace {

// the set-up waves of the look-up walk: in the walk's launch (p.fuse_setup) or in front of it
FusedSetupArgs fused_setup_args(const mi_engine* e, const DeviceCall& d, const CallPlan& p) {
  FusedSetupArgs fs{};
  fs.ts = tree_setup_args(e, d, p);
  fs.ms = model_setup_args(e, d, p);
  fs.mmats = e->mmats.as<double>();
  fs.colocate = e->sw.fused_colocate;
  if (p.fuse_setup) {
    fs.ready = e->ready.as<int32_t>();
    fs.debug_skip = e->sw.fused_debug_skip;
    fs.spin_ticks = e->sw.fused_spin_ticks;
    fs.fence = e->sw.fused_fence;
  }
  return fs;
}

// node-ordered matrices of every evaluation a log-likelihood or HBM kernel walks
TransitionArgs transition_args(const mi_engine* e, const DeviceCall& d, const CallPlan& p) {
  TransitionArgs tr{};
  tr.E = p.E;
  tr.N = e->N;
  tr.K = e->K;
  tr.map = EvalMap{d.T, p.models_per_tree};
  tr.models = e->models.as<DevModel>();
  tr.bl_eff = e->bl_eff.as<double>();
  tr.mats = e->mats.as<double>();
  tr.tip_tables = p.need_tip_tables ? e->tip_tables.as<double>() : nullptr;
  tr.n = e->n;
  // evaluations nobody walks need no matrices at all
  if (p.kind == kGradientCall && p.gtr && !p.analytic && !p.light && !p.fd_pass) {
    tr.ev_skip_begin = d.T;
    tr.ev_skip_end = p.site_pass ? 17 * d.T : p.E;
  }
  return tr;
}

// macro-ordered matrices of gradient evaluations [eval_begin, eval_begin + count), the
// grad_begin-th and following of the call's gradient workspace
TransitionMacroArgs transition_macro_args(const mi_engine* e, const DeviceCall& d, const CallPlan& p,
                                          int eval_begin, int grad_begin, int count) {
  TransitionMacroArgs tm{};
  tm.n = e->n;
  tm.N = e->N;
  tm.K = e->K;
  tm.count = count;
  tm.eval_begin = eval_begin;
  tm.map = EvalMap{d.T, p.models_per_tree};
  tm.models = e->models.as<DevModel>();
  tm.bl_eff = e->bl_eff.as<double>();
  tm.macros = walk_macros(e, p);
  tm.macro_count = e->macro_count.as<int32_t>();
  const size_t per = (p.walk3 ? gradient_walk_lut_mats_bytes_per_eval(e->n)
                              : gradient_walk_mats_bytes_per_eval(e->n, e->K)) / sizeof(double);
  tm.mmats = e->mmats.as<double>() + (size_t)grad_begin * per;
  tm.mphi = p.analytic ? e->mphi.as<double>() + (size_t)grad_begin * (per / 2) : nullptr;
  return tm;
}

LikArgs lik_args(const mi_engine* e, const DeviceCall& d, const CallPlan& p) {
  LikArgs la{};
  la.n = e->n;
  la.N = e->N;
  la.P = e->P;
  la.K = e->K;
  la.tiles = e->tiles;
  la.ll_tiles = e->ll_stride;
  la.g_tiles = p.g_tiles;
  la.map = EvalMap{d.T, p.models_per_tree};
  la.models = e->models.as<DevModel>();
  la.sched = e->sched.as<SchedEntry>();
  la.macros = walk_macros(e, p);
  la.macro_count = e->macro_count.as<int32_t>();
  la.mats = e->mats.as<double>();
  la.mmats = e->mmats.as<double>();
  la.tip_states = e->tip_states.as<int8_t>();
  la.tip_masks = e->have_tip_masks ? e->tip_masks.as<uint8_t>() : nullptr;
  la.tip_partials = e->spec.use_tip_states ? nullptr : e->tip_partials.as<double>();
  la.weights = e->weights.as<double>();
  la.ll_part = e->ll_part.as<double>();
  la.plv = e->plv.as<double>();
  la.g_part = e->g_part.as<double>();
  la.status = e->status.as<int32_t>();
  la.slot_need = e->slot_need.as<int32_t>();
  la.store = p.store;  // (the launchers follow the choice the schedules were made for)
  if (p.kind == kAncestralCall) {
    la.anc_state = d.out_anc_state;
    la.anc_map = d.out_anc_map;
    la.anc_cat = d.out_anc_cat;
    la.anc_rate = d.out_anc_rate;
    la.anc_tip = d.out_anc_tip;
    return la;
  }
  if (p.kind == kPlacementCall) {
    la.place_half = e->place_half.as<double>();
    la.place_pend = e->place_pend.as<double>();
    la.place_table = e->place_table.as<double>();
    la.place_G = d.G;
    return la;
  }
  if (p.kind == kHessianCall || p.kind == kNniCall || p.kind == kSprCall) return la;  // (their kernels read none of the following)
  la.tip_tables = e->tip_tables.as<double>();
  la.mphi = e->mphi.as<double>();
  // (MI_PHYLO_TIP_TILES=0: the kernels stage their tip bytes from tip_masks / tip_codes themselves
  // -- A/B, tests; the look-up walk's pre-tiled codes were made for the engine's tile width)
  la.tip_code_tiles = e->have_tip_codes && e->tip_code_tiles.ptr && e->sw.tip_tiles && e->tile_regs == p.tile_regs
                          ? e->tip_code_tiles.as<uint8_t>() : nullptr;
  la.tip_tiles = e->have_tip_masks && e->tip_tiles.ptr && e->sw.tip_tiles ? e->tip_tiles.as<uint8_t>() : nullptr;
  la.tip_codes = e->have_tip_codes ? e->tip_codes.as<uint8_t>() : nullptr;
  la.tile_regs = p.tile_regs;
  la.pattern_ll = p.pattern_ll ? d.out_pattern_ll : nullptr;
  la.pattern_blank = e->pattern_blank.as<uint8_t>();
  return la;
}

// arena calls whose set-up launch did not assign the LDS slots: the pass of its own
void macro_slots(const mi_engine* e, int T, hipStream_t s) {
  launch_macro_slots(e->macros.as<MacroEntry>(), e->arena_macros.as<MacroEntry>(),
                     e->macro_count.as<int32_t>(), e->n, T, e->slot_need.as<int32_t>(),
                     e->status.as<int32_t>(), e->sw, s);
}

// bookkeeping of a call: what mi_engine_last_call_* report
void note_call(mi_engine* e, const CallPlan& p, int first_launch_evals, int walk_launches) {
  e->dominant = p.dominant;
  e->last_path = plan_path(e, p);
  e->prof_first_launch_evals = first_launch_evals;
  e->last_evals = p.E;
  e->last_grad_evals = p.Eg;
  e->last_walk_launches = walk_launches;
}

int check_call(const mi_engine* e, const DeviceCall& d, const void* output) {
  if (d.T <= 0) return fail("tree_count must be positive");
  if (!d.parent_ids || !d.bl || !output) return fail("null tree / output pointer");
  if (e->param_count > 0 && !d.params) return fail("null parameter matrix");
  return 0;
}

}  // namespace

// Enqueue one engine call; every pointer in `d` is a device pointer.
int run_device(mi_engine* e, hipStream_t s, const DeviceCall& d_in) {
  // (a caller driving several GPUs from one thread may have another device current)
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return d_in.out_pattern_ll ? fail(kPatternLl4State) : aa_run_device(e, s, d_in);
  if (check_call(e, d_in, d_in.out_pattern_ll ? d_in.out_pattern_ll : d_in.out_ll)) return 1;
  const CallPlan p = plan_call(e, d_in.gradient ? kGradientCall : kLogLikCall, d_in);
  if (reserve(e, p)) return 1;
  DeviceCall d = d_in;
  if (!d.out_ll) d.out_ll = e->pattern_ll_out.as<double>();  // (the per-pattern call: nobody wants the sums)
  const int n = e->n, N = e->N, T = d.T;
  // (the status word is sticky: cleared when it is read, check_status -- not per call: one
  // dispatch less on the small-batch path)
  const bool prof = e->prof_used < e->prof_capacity;
  const bool marks = prof && e->prof_phases;
  PROF_MARK(e, marks, 0, s);

  // set-up: tree schedules and model instances, one launch (or riding with the walk's records)
  if (p.setup_records) launch_setup_records(fused_setup_args(e, d, p), T, s);
  if (p.setup_wg) launch_setup_workgroups(fused_setup_args(e, d, p), T, s);
  const bool slots_done = !p.fuse_setup && !p.setup_records && !p.setup_wg &&
                          launch_setup(tree_setup_args(e, d, p), model_setup_args(e, d, p), e->sw, s);
  if (p.store == kStoreArena && !slots_done) macro_slots(e, T, s);

  // matrices
  TransitionArgs tr = transition_args(e, d, p);
  if (p.mfma && p.groups == 1) {
    // the walks read their matrices in macro order (below); node-ordered ones are only needed
    // by the evaluations a log-likelihood kernel walks: the finite-difference passes
    // [T, 17 T) of a GTR call
    if (p.fd_pass) {
      tr.eval_base = T;
      tr.E = 16 * T;
      launch_transition(tr, s);
    }
  } else {
    launch_transition(tr, s);
  }
  auto macro_matrices = [&](int eval_begin, int grad_begin, int count) {
    const TransitionMacroArgs tm = transition_macro_args(e, d, p, eval_begin, grad_begin, count);
    if (p.walk3) launch_transition_lut(tm, s);
    else launch_transition_macro(tm, s);
  };
  if (p.mfma && !p.fuse_setup && !p.setup_records && !p.setup_wg) {
    macro_matrices(0, 0, T);
    if (p.site_pass) macro_matrices(17 * T, T, T);
  }

  // walk
  const LikArgs la = lik_args(e, d, p);
  int walk_launches = 0;
  auto loglik_range = [&](int eval_begin, int count) {
    launch_in_parts(e, count, 0, walk_launches, [&](int done, int part) {
      LikArgs l = la;
      l.eval_offset = eval_begin + done;
      launch_loglik(l, part, d.rescaling, e->max_slots, e->sw, s);
    });
  };
  auto grad_range = [&](int eval_begin, int grad_begin, int count) {
    // (arena variant, HBM kernel: a launch covers what its HBM arena holds)
    launch_in_parts(e, count, vector_bytes_per_eval(e, p), walk_launches, [&](int done, int part) {
      LikArgs g = la;
      g.eval_offset = eval_begin + done;
      g.grad_offset = grad_begin + done;
      if (!p.mfma) return launch_gradient_hbm(g, part, d.rescaling, s);
      if (p.groups > 1) {
        // K > 4: the site likelihoods (and logL) come from a log-likelihood pass
        g.site_lik = e->site_lik.as<double>();
        g.site_exp = e->site_exp.as<int32_t>();
        launch_loglik(g, part, d.rescaling, e->max_slots, e->sw, s);
      }
      if (p.fuse_setup) launch_gradient_walk_lut_fused(g, fused_setup_args(e, d, p), part, d.rescaling, s);
      else if (p.walk3) launch_gradient_walk_lut(g, part, d.rescaling, e->sw, s);
      else launch_gradient_walk(g, part, d.rescaling, p.analytic, e->sw, s);
    });
  };
  if (prof) HIP_TRY(hipEventRecord(prof_event(e, 0), s));
  PROF_MARK(e, marks, 1, s);
  PROF_MARK(e, marks, 2, s);
  if (!d.gradient) {
    loglik_range(0, T);
    if (prof) HIP_TRY(hipEventRecord(prof_event(e, 1), s));
    PROF_MARK(e, marks, 3, s);
  } else {
    grad_range(0, 0, T);
    if (prof) HIP_TRY(hipEventRecord(prof_event(e, 1), s));
    PROF_MARK(e, marks, 3, s);
    if (p.fd_pass) loglik_range(T, 16 * T);
    if (p.site_pass) grad_range(17 * T, T, T);
  }
  note_call(e, p, T, walk_launches);

  // reduce / finalize
  FinalizeArgs fa = finalize_args(e, d);
  fa.ll_tiles = e->ll_stride;
  fa.g_tiles = p.g_tiles;
  fa.ll_part = e->ll_part.as<double>();
  fa.g_part = e->g_part.as<double>();
  // logL partial sums each evaluation's walk kernel wrote (no memset of ll_part: the
  // consumers sum exactly these): the log-likelihood kernel in use tiles the patterns its
  // way, the gradient kernels theirs; K > 4 takes the gradient evaluations' logL from the
  // log-likelihood pass
  const int ll_kernel_count = p.loglik_is_valu ? e->tiles : loglik_mfma_tiles(e->P, e->K);
  const int grad_kernel_count =
      p.mfma ? (p.groups > 1 ? ll_kernel_count : p.g_tiles) : e->tiles;
  LlCounts ll_used{d.gradient ? grad_kernel_count : ll_kernel_count, ll_kernel_count, 0, 0};
  if (d.gradient && p.gtr && !p.analytic && !p.light) {
    ll_used.mid_lo = T;
    ll_used.mid_hi = 17 * T;
  }
  fa.ll_used = ll_used;
  bool fused = false;
  ReduceArgs ra{};
  if (reduce_tiles_fits(N)) {
    // sum the per-tile partials with one workgroup per evaluation first
    ra.N = N;
    ra.E = p.E;
    ra.Eg = p.Eg;
    ra.ll_tiles = e->ll_stride;
    ra.ll_used = ll_used;
    ra.g_tiles = p.g_tiles;
    ra.ll_part = e->ll_part.as<double>();
    ra.g_part = e->g_part.as<double>();
    ra.ll_sum = e->ll_sum.as<double>();
    ra.g_sum = e->g_sum.as<double>();
    ra.g_width = p.mfma ? gradient_mfma_width(n, p.analytic) : 0;
    ra.extra = p.analytic ? kSubstExtra : 0;
    ra.x_sum = e->x_sum.as<double>();
    ra.n = n;
    ra.T = T;
    ra.macros = walk_macros(e, p);
    ra.macro_count = e->macro_count.as<int32_t>();
    // one evaluation per tree (JC69-type models, the analytic GTR gradient; log-likelihood
    // calls too): tile reduction and finalize step in ONE launch, a workgroup per tree
    fused = e->sw.fuse_finalize && p.E == T;
    if (!fused) launch_reduce_tiles(ra, s);
    fa.ll_tiles = 1;
    fa.ll_used = LlCounts{1, 1, 0, 0};
    fa.g_tiles = 1;
    fa.ll_part = ra.ll_sum;
    fa.g_part = ra.g_sum;
  }
  fa.gtr = p.gtr && !p.analytic && !p.light;  // finite-difference assembly of the substitution gradient
  fa.site_fused = p.site_fused;
  fa.site_separate = p.site_separate;
  fa.out_subst = d.out_subst;
  fa.clear_ready = p.fuse_setup ? e->ready.as<int32_t>() : nullptr;
  if (p.fuse_setup && !fused) return fail("internal error: the one-launch call needs the fused reduction");
  if (fused) launch_reduce_finalize(ra, fa, s);
  else launch_finalize(fa, s);
  if (p.analytic && d.out_subst) {
    SubstGradArgs sg{};
    sg.T = T;
    sg.param_count = e->param_count;
    sg.rates_off = e->rates_off;
    sg.freqs_off = e->freqs_off;
    sg.params = d.params;
    sg.models = e->models.as<DevModel>();
    sg.x_sum = e->x_sum.as<double>();
    sg.out_subst = d.out_subst;
    launch_subst_gradient(sg, s);
  }
  PROF_MARK(e, marks, 4, s);
  if (prof) e->prof_used++;
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- the calls of the HBM-streamed kernel family ----
// One evaluation per tree with the tree's own model, the node-ordered matrices, the member's
// kernel over the vector arena in parts, one finalize launch: the Hessian call where no
// matrix-core walk takes it, the NNI scan, the ancestral-state call, placement, the SPR scan.
// (trees, models, node-ordered matrices, log-likelihood partials: the Hessian call's walk form too)
static int reserve_per_tree(mi_engine* e, int T) {
  const int n = e->n, N = e->N;
  if (e->tree_scratch.ensure(sizeof(int32_t) * (size_t)T * 13 * N)) return 1;
  if (e->sched.ensure(sizeof(SchedEntry) * (size_t)T * (n - 1))) return 1;
  if (e->macro_count.ensure(sizeof(int32_t) * (size_t)T)) return 1;
  if (e->bl_eff.ensure(sizeof(double) * (size_t)T * N)) return 1;
  if (e->models.ensure(sizeof(DevModel) * (size_t)T)) return 1;
  if (e->mats.ensure(sizeof(double) * (size_t)T * (N - 1) * e->K * 16)) return 1;
  if (e->ll_part.ensure(sizeof(double) * (size_t)T * e->ll_stride)) return 1;
  return e->status.ensure(sizeof(int32_t) * kStatusWords);
}
// What every such call needs; g_width: doubles of g_part per (tree, tile), 0: the kernel has none.
static int reserve_hbm_family(mi_engine* e, int T, int g_width) {
  const size_t per = plv_bytes_per_eval(e);
  const size_t chunk = std::max<size_t>(1, std::min<size_t>(T, e->plv_budget / per));
  if (e->plv.ensure(per * chunk)) return 1;
  if (g_width && e->g_part.ensure(sizeof(double) * (size_t)T * e->tiles * g_width)) return 1;
  return reserve_per_tree(e, T);
}
// The sequence of a call with one evaluation per tree, after check, plan and reservation:
// prepare() -- set-up and matrices --, launch(args, count, rescale, stream) over the vector arena
// in parts, finalize().
template <typename Prepare, typename Launch, typename Finalize>
int run_per_tree_call(mi_engine* e, hipStream_t s, const DeviceCall& d, const CallPlan& p, Prepare prepare,
                      Launch launch, Finalize finalize) {
  const int T = d.T;
  const bool prof = e->prof_used < e->prof_capacity;
  const bool marks = prof && e->prof_phases;
  PROF_MARK(e, marks, 0, s);
  prepare();

  const LikArgs la = lik_args(e, d, p);
  if (prof) HIP_TRY(hipEventRecord(prof_event(e, 0), s));
  PROF_MARK(e, marks, 1, s);
  PROF_MARK(e, marks, 2, s);
  // (a launch covers what the vector arena holds)
  int walk_launches = 0;
  const int first = launch_in_parts(e, T, vector_bytes_per_eval(e, p), walk_launches, [&](int done, int part) {
    LikArgs g = la;
    g.eval_offset = done;
    g.grad_offset = done;
    launch(g, part, d.rescaling, s);
  });
  if (prof) HIP_TRY(hipEventRecord(prof_event(e, 1), s));
  PROF_MARK(e, marks, 3, s);
  finalize();
  PROF_MARK(e, marks, 4, s);
  if (prof) e->prof_used++;
  note_call(e, p, first, walk_launches);
  HIP_TRY(hipGetLastError());
  return 0;
}
// ... of a member of the HBM-streamed family: set-up, node-ordered matrices
template <typename Launch, typename Finalize>
int run_hbm_family(mi_engine* e, hipStream_t s, const DeviceCall& d, const CallPlan& p, Launch launch,
                   Finalize finalize) {
  auto prepare = [&] {
    launch_setup(tree_setup_args(e, d, p), model_setup_args(e, d, p), e->sw, s);
    launch_transition(transition_args(e, d, p), s);
  };
  return run_per_tree_call(e, s, d, p, prepare, launch, finalize);
}

// ---- the branch-length Hessian call (mi_engine_branch_hessian_unrooted*) ----
// The Hessian form of the second-generation walk with its macro-ordered matrices, or of the
// HBM-streamed gradient kernel (plan_call); one launch reduces the tiles and writes the outputs.
int reserve_hessian(mi_engine* e, const CallPlan& p) {
  const int n = e->n, T = p.T;
  if (!p.mfma) return reserve_hbm_family(e, T, 3 * e->N);
  if (e->macros.ensure(sizeof(MacroEntry) * (size_t)T * macro_stride(n))) return 1;
  if (e->mmats.ensure(gradient_walk_mats_bytes_per_eval(n, e->K) * (size_t)T)) return 1;
  if (e->g_part.ensure(sizeof(double) * (size_t)T * p.g_tiles * max_macros(n) * kMacroPositions * 3)) return 1;
  if (p.reserve_arena) {
    const size_t aper = gradient_arena_bytes_per_eval(n, e->P, e->K);
    const size_t achunk = std::max<size_t>(1, std::min<size_t>(T, e->plv_budget / aper));
    if (e->plv.ensure(aper * achunk)) return 1;
    if (e->arena_macros.ensure(sizeof(MacroEntry) * (size_t)T * macro_stride(n))) return 1;
    if (e->slot_need.ensure(sizeof(int32_t) * (size_t)T)) return 1;
  }
  return reserve_per_tree(e, T);
}
// (both rescaling settings: a later *_device call of either allocates nothing)
int reserve_hessian_calls(mi_engine* e, int T) {
  return reserve_hessian(e, plan_call(e, kHessianCall, T, false)) || reserve_hessian(e, plan_call(e, kHessianCall, T, true));
}

int run_hessian_device(mi_engine* e, hipStream_t s, const DeviceCall& d) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return fail(kHessian4State);
  if (check_call(e, d, d.out_hess)) return 1;
  const CallPlan p = plan_call(e, kHessianCall, d);
  if (reserve_hessian(e, p)) return 1;
  const int n = e->n, N = e->N, T = d.T;
  auto finalize = [&] {
    HessFinalizeArgs fa{};
    fa.N = N;
    fa.T = T;
    fa.g_tiles = p.g_tiles;
    fa.ll_tiles = e->ll_stride;
    fa.ll_used = p.g_tiles;
    fa.n = n;
    fa.g_width = p.mfma ? max_macros(n) * kMacroPositions * 3 : 3 * N;
    fa.macros = p.mfma ? walk_macros(e, p) : nullptr;
    fa.macro_count = e->macro_count.as<int32_t>();
    fa.ll_part = e->ll_part.as<double>();
    fa.g_part = e->g_part.as<double>();
    fa.out_ll = d.out_ll;
    fa.out_branch = d.out_branch;
    fa.out_hess = d.out_hess;
    fa.out_gsq = d.out_gsq;
    launch_hessian_finalize(fa, s);
  };
  if (!p.mfma) return run_hbm_family(e, s, d, p, launch_gradient_hbm_hessian, finalize);
  // the walk form: LDS slots of the arena variant, macro-ordered matrices
  auto prepare = [&] {
    const bool slots_done = launch_setup(tree_setup_args(e, d, p), model_setup_args(e, d, p), e->sw, s);
    if (p.store == kStoreArena && !slots_done) macro_slots(e, T, s);
    launch_transition_macro(transition_macro_args(e, d, p, 0, 0, T), s);
  };
  return run_per_tree_call(e, s, d, p, prepare, launch_gradient_walk_hessian, finalize);
}

// ---- the NNI neighbourhood scan (mi_engine_nni_scan_unrooted*) ----
// The scan kernel; one launch reduces the tiles and writes logL, delta and the best move.
// (the plan does not depend on the rescaling setting: one reservation serves both)
int reserve_nni_calls(mi_engine* e, int T) { return reserve_hbm_family(e, T, 2 * e->N); }

int run_nni_device(mi_engine* e, hipStream_t s, const DeviceCall& d) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return fail(kNni4State);
  if (check_call(e, d, d.out_nni)) return 1;
  const CallPlan p = plan_call(e, kNniCall, d);
  if (reserve_nni_calls(e, d.T)) return 1;
  return run_hbm_family(e, s, d, p, launch_nni_scan_hbm, [&] {
    NniFinalizeArgs fa{};
    fa.N = e->N;
    fa.n = e->n;
    fa.T = d.T;
    fa.g_tiles = p.g_tiles;
    fa.ll_tiles = e->ll_stride;
    fa.ll_used = p.g_tiles;
    fa.ll_part = e->ll_part.as<double>();
    fa.g_part = e->g_part.as<double>();
    fa.out_ll = d.out_ll;
    fa.out_delta = d.out_nni;
    fa.out_best = d.out_best;
    launch_nni_finalize(fa, s);
  });
}

// ---- ancestral-state and rate-category posteriors (mi_engine_ancestral_states_unrooted*) ----
// The kernel writes the posteriors itself, by the call's tree index; one launch sums the tiles'
// log-likelihood partials when the caller wants the log-likelihoods.
// (the plan does not depend on the rescaling setting: one reservation serves both)
int reserve_ancestral_calls(mi_engine* e, int T) { return reserve_hbm_family(e, T, 0); }

int run_ancestral_device(mi_engine* e, hipStream_t s, const DeviceCall& d) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return fail(kAncestral4State);
  if (check_call(e, d, d.out_anc_state)) return 1;
  const CallPlan p = plan_call(e, kAncestralCall, d);
  if (reserve_ancestral_calls(e, d.T)) return 1;
  return run_hbm_family(e, s, d, p, launch_ancestral_hbm, [&] {
    launch_ancestral_finalize(e->ll_part.as<double>(), d.T, e->ll_stride, p.g_tiles, d.out_ll, s);
  });
}

// ---- placement (mi_engine_placement_unrooted*) ----
// The table kernel over the vector arena in parts, as every member; inside a part, over what the
// table workspace holds: table launch, scoring launch (and the copy of the table, if wanted) per
// sub-part.  One launch at the end for best edges, weight ratios and log-likelihoods.  The
// half-length and pendant matrices are two more launches of the transition kernel, in front of
// the first table launch (the effective lengths exist once the set-up launch has run).
int check_placement_shape(const mi_engine* e, int Q, int C, int G) {
  if (Q < 1) return fail("placement: query_count must be positive");
  if (C < 1) return fail("placement: column_count must be positive");
  if (G < 1 || G > kPlacementMaxPendants)
    return fail("placement: pendant_count must be in [1, " + std::to_string(kPlacementMaxPendants) + "]");
  return 0;
}

static size_t placement_table_bytes_per_tree(const mi_engine* e, int G) {
  return sizeof(double) * (size_t)(2 * e->n - 3) * G * 5 * e->tiles * kTile;
}
// trees a table launch covers: what the budget holds
static int placement_table_trees(const mi_engine* e, int T, int G) {
  return (int)std::max<size_t>(1, std::min<size_t>(T, e->plv_budget / placement_table_bytes_per_tree(e, G)));
}

int reserve_placement_calls(mi_engine* e, int T, int G) {
  const int N = e->N;
  const size_t per = placement_table_bytes_per_tree(e, G);
  if (per > e->plv_budget)
    return fail("placement: the table of one tree (" + std::to_string(per) + " bytes: 2n-3 edges x " +
                std::to_string(G) + " pendant lengths x 5 x padded patterns x 8) exceeds the arena budget (" +
                std::to_string(e->plv_budget) + " bytes, MI_PHYLO_PLV_BYTES)");
  if (e->place_bl.ensure(sizeof(double) * (size_t)T * (N + kPlacementMaxPendants + 1))) return 1;
  if (e->place_half.ensure(sizeof(double) * (size_t)T * (N - 1) * e->K * 16)) return 1;
  if (e->place_pend.ensure(sizeof(double) * (size_t)T * kPlacementMaxPendants * e->K * 16)) return 1;
  if (e->place_table.ensure(per * placement_table_trees(e, T, G))) return 1;
  return reserve_hbm_family(e, T, 0);
}

int run_placement_device(mi_engine* e, hipStream_t s, const DeviceCall& d) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return fail(kPlacement4State);
  if (check_call(e, d, d.out_place_edge_ll)) return 1;
  if (check_placement_shape(e, d.Q, d.C, d.G)) return 1;
  const CallPlan p = plan_call(e, kPlacementCall, d);
  if (reserve_placement_calls(e, d.T, d.G)) return 1;
  const int T = d.T, N = e->N, G = d.G, E = 2 * e->n - 3;
  const size_t ppad = (size_t)e->tiles * kTile;
  const int table_trees = placement_table_trees(e, T, G);
  double* half_bl = e->place_bl.as<double>();
  double* pend_bl = half_bl + (size_t)T * N;
  int table_launches = 0;
  const int rc = run_hbm_family(
      e, s, d, p,
      [&](const LikArgs& g, int part, bool rescale, hipStream_t s) {
        if (g.eval_offset == 0) {
          PlacePrepareArgs pa{};
          pa.T = T, pa.N = N, pa.G = G, pa.C = d.C, pa.P = e->P;
          pa.bl_eff = e->bl_eff.as<double>();
          pa.pendant_lengths = d.pendant_lengths;
          pa.column_pattern = d.column_pattern;
          pa.half_bl = half_bl;
          pa.pend_bl = pend_bl;
          pa.status = e->status.as<int32_t>();
          launch_placement_prepare(pa, s);
          TransitionArgs tr = transition_args(e, d, p);
          tr.bl_eff = half_bl;
          tr.mats = e->place_half.as<double>();
          launch_transition(tr, s);
          tr.N = G + 1;  // (G "edges" per tree: the pendant branches)
          tr.bl_eff = pend_bl;
          tr.mats = e->place_pend.as<double>();
          launch_transition(tr, s);
        }
        for (int done = 0; done < part; done += table_trees) {
          const int count = std::min(table_trees, part - done);
          LikArgs h = g;
          h.eval_offset = g.eval_offset + done;
          h.grad_offset = h.eval_offset;
          h.place_tree0 = h.eval_offset;
          launch_placement_table_hbm(h, count, rescale, s);
          table_launches++;
          PlaceScoreArgs sa{};
          sa.trees = count, sa.tree0 = h.eval_offset;
          sa.E = E, sa.G = G, sa.P = e->P, sa.Q = d.Q, sa.C = d.C;
          sa.ppad = ppad;
          sa.use_lds = !e->sw.place_table_global && placement_table_fits_lds(G, ppad);
          sa.table = e->place_table.as<double>();
          sa.query_states = d.query_states;
          sa.column_pattern = d.column_pattern;
          sa.column_weights = d.column_weights;
          sa.edge_ll = d.out_place_edge_ll;
          sa.pendant_index = d.out_place_pendant;
          launch_placement_score(sa, s);
          if (d.out_place_tables)
            launch_placement_table_copy(sa.table, count, sa.tree0, E, G, e->P, ppad, d.out_place_tables, s);
        }
      },
      [&] {
        PlaceFinalizeArgs fa{};
        fa.T = T, fa.Q = d.Q, fa.E = E;
        fa.ll_tiles = e->ll_stride;
        fa.ll_used = p.g_tiles;
        fa.ll_part = e->ll_part.as<double>();
        fa.edge_ll = d.out_place_edge_ll;
        fa.out_ll = d.out_ll;
        fa.out_best_edge = d.out_place_best;
        fa.out_lwr = d.out_place_lwr;
        launch_placement_finalize(fa, s);
      });
  if (rc == 0) e->last_walk_launches = table_launches;
  return rc;
}

// ---- the SPR neighbourhood scan (mi_engine_spr_scan_unrooted*) ----
// The vectors kernel over the vector arena in parts, as every member; inside a part, over what the
// scan's own workspace holds: vectors, regraft walk and finalize launch per sub-part (the finalize
// launch writes the sub-part's trees, log-likelihoods included: nothing is left for the end).
// The half-length matrices are one more launch of the transition kernel in front of the first.
int check_spr_shape(const mi_engine* e, int radius) {
  if (radius < 0) return fail("SPR scan: radius must be 0 (every move) or positive, not " + std::to_string(radius));
  if (!spr_regraft_fits_lds(e->n, e->n))
    return fail("SPR scan: a tree of " + std::to_string(e->n) + " taxa does not fit the regraft walk's LDS");
  return 0;
}

namespace {
// what one tree of a launch holds in spr_ws: doubles (second arena, L_p, partial table), int32s
// (exponents below, exponents above, that of L_p)
struct SprLayout {
  size_t ppad, up, site, part, exp_down, exp_up, site_exp;  // elements per tree
  size_t doubles() const { return up + site + part; }
  size_t ints() const { return exp_down + exp_up + site_exp; }
  size_t bytes() const { return sizeof(double) * doubles() + sizeof(int32_t) * ints(); }
};
SprLayout spr_layout(const mi_engine* e) {
  SprLayout l;
  const size_t n = e->n, E = 2 * n - 3;
  l.ppad = (size_t)e->tiles * kTile;
  l.up = (2 * n - 2) * e->K * l.ppad * 4;
  l.site = l.ppad;
  l.part = (size_t)e->tiles * 2 * E * E;
  l.exp_down = (n - 1) * l.ppad;
  l.exp_up = (2 * n - 2) * l.ppad;
  l.site_exp = l.ppad;
  return l;
}
// trees a launch covers: what the budget holds
int spr_launch_trees(const mi_engine* e, int T) {
  return (int)std::max<size_t>(1, std::min<size_t>(T, e->plv_budget / spr_layout(e).bytes()));
}
// The regraft waves' paths: a wave per job (tree, tile, pruned edge) of a call of T trees, at most
// kSprWaves waves, fewer where a path of n messages is long (1 GiB in all).
constexpr int kSprWaves = 2048;
size_t spr_path_bytes_per_wave(const mi_engine* e, int slots) {
  return sizeof(double) * (size_t)(slots + 1) * e->K * kTile * 4 + sizeof(int32_t) * (size_t)slots * kTile;
}
int spr_waves(const mi_engine* e, int T) {
  const size_t jobs = (size_t)T * e->tiles * (2 * (size_t)e->n - 3);
  const size_t fit = ((size_t)1 << 30) / spr_path_bytes_per_wave(e, e->n);
  return (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(kSprWaves, jobs), fit));
}
}  // namespace

int reserve_spr_calls(mi_engine* e, int T) {
  const int N = e->N;
  const size_t per = spr_layout(e).bytes();
  if (per > e->plv_budget)
    return fail("SPR scan: the workspace of one tree (" + std::to_string(per) + " bytes: second arena, exponents and "
                "the per-tile table of 2 (2n-3)^2 moves) exceeds the arena budget (" + std::to_string(e->plv_budget) +
                " bytes, MI_PHYLO_PLV_BYTES)");
  if (e->spr_bl.ensure(sizeof(double) * (size_t)T * N)) return 1;
  if (e->spr_half.ensure(sizeof(double) * (size_t)T * (N - 1) * e->K * 16)) return 1;
  if (e->spr_ws.ensure(per * spr_launch_trees(e, T))) return 1;
  if (e->spr_path.ensure(spr_path_bytes_per_wave(e, e->n) * spr_waves(e, T))) return 1;
  return reserve_hbm_family(e, T, 0);
}

int run_spr_device(mi_engine* e, hipStream_t s, const DeviceCall& d) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return fail(kSpr4State);
  if (check_spr_shape(e, d.spr_radius)) return 1;
  if (check_call(e, d, d.out_spr_target)) return 1;
  if (!d.out_spr_delta) return fail("null best-delta output");
  const CallPlan p = plan_call(e, kSprCall, d);
  if (reserve_spr_calls(e, d.T)) return 1;
  const int T = d.T, n = e->n, N = e->N;
  const int launch_trees = spr_launch_trees(e, T);
  const SprLayout l = spr_layout(e);
  SprArgs base{};
  base.n = n, base.K = e->K, base.P = e->P, base.tiles = e->tiles;
  base.radius = d.spr_radius;
  base.depth_slots = d.spr_radius ? std::min(n, d.spr_radius) : n;
  base.waves = spr_waves(e, T);
  base.ll_tiles = e->ll_stride, base.ll_used = p.g_tiles;
  base.models = e->models.as<DevModel>();
  base.sched = e->sched.as<SchedEntry>();
  base.mats = e->mats.as<double>();
  base.half = e->spr_half.as<double>();
  base.weights = e->weights.as<double>();
  base.tip_states = e->tip_states.as<int8_t>();
  base.tip_partials = e->spec.use_tip_states ? nullptr : e->tip_partials.as<double>();
  base.down = e->plv.as<double>();
  base.up = e->spr_ws.as<double>();
  base.site = base.up + l.up * launch_trees;
  base.part = base.site + l.site * launch_trees;
  base.exp_down = reinterpret_cast<int32_t*>(base.part + l.part * launch_trees);
  base.exp_up = base.exp_down + l.exp_down * launch_trees;
  base.site_exp = base.exp_up + l.exp_up * launch_trees;
  base.path = e->spr_path.as<double>();
  base.path_exp = reinterpret_cast<int32_t*>(base.path + (size_t)base.waves * (base.depth_slots + 1) * e->K * kTile * 4);
  base.ll_part = e->ll_part.as<double>();
  base.out_ll = d.out_ll;
  base.out_best_target = d.out_spr_target;
  base.out_best_delta = d.out_spr_delta;
  base.out_best_move = d.out_spr_move;
  base.out_delta = d.out_spr_table;
  int launches = 0;
  const int rc = run_hbm_family(
      e, s, d, p,
      [&](const LikArgs& g, int part, bool rescale, hipStream_t s) {
        if (g.eval_offset == 0) {
          launch_spr_half_lengths(e->bl_eff.as<double>(), (size_t)T * N, e->spr_bl.as<double>(), s);
          TransitionArgs tr = transition_args(e, d, p);
          tr.bl_eff = e->spr_bl.as<double>();
          tr.mats = e->spr_half.as<double>();
          launch_transition(tr, s);
        }
        for (int done = 0; done < part; done += launch_trees) {
          LikArgs h = g;
          h.eval_offset = g.eval_offset + done;
          h.grad_offset = h.eval_offset;
          SprArgs w = base;
          w.trees = std::min(launch_trees, part - done);
          w.tree0 = h.eval_offset;
          launch_spr_vectors_hbm(h, w, w.trees, rescale, s);
          launch_spr_regraft(w, rescale, s);
          launch_spr_finalize(w, s);
          launches++;
        }
      },
      [] {});
  if (rc == 0) e->last_walk_launches = launches;
  return rc;
}
