// The one reader of the MI_PHYLO_* environment switches (mi_phylo_switches.h; README lists them).
#include "mi_phylo_switches.h"

#include <cerrno>
#include <climits>
#include <cstdlib>
#include <cstring>

namespace miphylo {
namespace {

struct Reader {
  std::string error;

  const char* get(const char* name) {
    const char* v = getenv(name);
    return v && *v ? v : nullptr;
  }
  void reject(const char* name, const char* value, const std::string& expected) {
    if (error.empty()) error = std::string(name) + "=" + value + ": expected " + expected;
  }
  // one of the words of `values` ("a|b|c"): its index; unset: `dflt`
  int choice(const char* name, const char* values, int dflt) {
    const char* v = get(name);
    if (!v) return dflt;
    const size_t len = strlen(v);
    int index = 0;
    for (const char* w = values;; index++) {
      const char* end = strchr(w, '|');
      const size_t wlen = end ? (size_t)(end - w) : strlen(w);
      if (wlen == len && strncmp(w, v, len) == 0) return index;
      if (!end) break;
      w = end + 1;
    }
    reject(name, v, values);
    return dflt;
  }
  bool on_off(const char* name, bool dflt) { return choice(name, "0|1", dflt ? 1 : 0) == 1; }
  // one of the numbers of `values` ("1|2|4"); unset: `dflt`
  int listed(const char* name, const char* values, int dflt) {
    return choice(name, values, -1) < 0 ? dflt : atoi(get(name));
  }
  long long integer(const char* name, long long lo, long long hi, long long dflt) {
    const char* v = get(name);
    if (!v) return dflt;
    char* end = nullptr;
    errno = 0;
    const long long x = strtoll(v, &end, 10);
    if (end != v && *end == '\0' && errno == 0 && x >= lo && x <= hi) return x;
    reject(name, v, hi == LLONG_MAX ? "an integer >= " + std::to_string(lo)
                                    : "an integer in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
    return dflt;
  }
  double number(const char* name, double lo, double hi, const char* range, double dflt) {
    const char* v = get(name);
    if (!v) return dflt;
    char* end = nullptr;
    errno = 0;
    const double x = strtod(v, &end);
    if (end != v && *end == '\0' && errno == 0 && x >= lo && x <= hi) return x;
    reject(name, v, std::string("a number in ") + range);
    return dflt;
  }
};

}  // namespace

bool parse_switches(Switches& out, std::string& error) {
  Reader r;
  Switches s;
  s.hbm_gradient = r.choice("MI_PHYLO_GRADIENT_PATH", "mfma|hbm", 0) == 1;
  s.walk3 = r.choice("MI_PHYLO_GRADIENT_WALK", "v2|v3", 1) == 1;
  s.walk3_arena = r.on_off("MI_PHYLO_WALK3_ARENA", true);
  s.walk3_k1_lds = r.on_off("MI_PHYLO_WALK3_K1", true);
  s.gradient_store = r.choice("MI_PHYLO_GRADIENT_STORE", "lds|arena", -1) + 1;
  s.walk_tile_regs = r.listed("MI_PHYLO_WALK_TILE_REGS", "3|4", 0);
  s.walk_tiles_per_wave = (int)r.integer("MI_PHYLO_WALK_TILES_PER_WAVE", 1, INT_MAX, 0);
  s.arena_nt = r.listed("MI_PHYLO_ARENA_NT", "0|1", -1);
  s.tip_tiles = r.on_off("MI_PHYLO_TIP_TILES", true);
  s.analytic_subst = r.choice("MI_PHYLO_SUBST_GRADIENT", "fd|analytic", 0) == 1;
  s.loglik_path = r.choice("MI_PHYLO_LOGLIK_PATH", "valu|mfma", -1) + 1;
  s.loglik_evals_per_wave = r.listed("MI_PHYLO_LOGLIK_EVALS_PER_WAVE", "1|2|4|8", 0);
  s.tree_setup = r.choice("MI_PHYLO_TREE_SETUP", "small|wg|lds", -1) + 1;
  s.macro_slots = r.choice("MI_PHYLO_MACRO_SLOTS", "own|seq", -1) + 1;
  s.setup_records = r.choice("MI_PHYLO_SETUP_RECORDS", "0|1|wg", -1);
  s.fused_setup = r.on_off("MI_PHYLO_FUSED_SETUP", true);
  s.fuse_finalize = r.on_off("MI_PHYLO_FUSE_FINALIZE", true);
  s.fused_max_trees = (int)r.integer("MI_PHYLO_FUSED_MAX_TREES", 0, INT_MAX, 512);
  s.fused_fence = r.choice("MI_PHYLO_FUSED_FENCE", "none|l1|agent", 1);
  s.fused_colocate = r.on_off("MI_PHYLO_FUSED_COLOCATE", true);
  // (milliseconds -> ticks of the 100 MHz clock, at most 2e9)
  s.fused_spin_ticks = (int)(r.number("MI_PHYLO_FUSED_SPIN_MS", 0.01, 2.0e4, "[0.01, 20000]", 0.0) * 1.0e5);
  s.fused_debug_skip = (int)r.integer("MI_PHYLO_DEBUG_FUSED_SKIP", 0, INT_MAX, 0);
  s.plv_bytes = r.integer("MI_PHYLO_PLV_BYTES", 0, LLONG_MAX, -1);
  s.place_table_global = r.choice("MI_PHYLO_PLACE_TABLE", "lds|global", 0) == 1;
  s.boot_hist_global = r.choice("MI_PHYLO_BOOT_HIST", "lds|global", 0) == 1;
  s.split_hash_bits = (int)r.integer("MI_PHYLO_SPLIT_HASH_BITS", 0, 32, 32);
  s.sbn_trees_per_wave = r.listed("MI_PHYLO_SBN_TREES_PER_WAVE", "16|32|64", 16);
  s.gp_hybrid_z = (int)r.integer("MI_PHYLO_GP_HYBRID_Z", 0, 65535, 0);
  s.gp_trees_global = r.choice("MI_PHYLO_GP_TREES_STORE", "lds|global", 0) == 1;
  s.aa_jacobi_seq = r.choice("MI_PHYLO_AA_JACOBI", "wave|seq", 0) == 1;
  s.aa_post_wave = r.choice("MI_PHYLO_AA_POST", "wg|wave", 0) == 1;
  s.aa_pre_wave = r.choice("MI_PHYLO_AA_PRE", "wg|wave", 0) == 1;
  s.aa_post_tiles = r.listed("MI_PHYLO_AA_POST_TILES", "1|2|4", 0);
  s.aa_post_one_tile_below = (long)r.integer("MI_PHYLO_AA_POST_ONE_TILE_BELOW", 0, LONG_MAX, -1);
  s.aa_ring = r.listed("MI_PHYLO_AA_RING", "0|1|2|4", -1);
  s.aa_pre_ring = r.listed("MI_PHYLO_AA_PRE_RING", "0|1|2", -1);
  s.aa_lds_pad = (size_t)r.integer("MI_PHYLO_AA_LDS_PAD", 0, 160 * 1024, 0);
  error = r.error;
  if (!error.empty()) return false;
  out = s;
  return true;
}

}  // namespace miphylo
