// The engine's environment switches (README, "Environment switches"): every MI_PHYLO_* variable
// the library reads, parsed in ONE place (mi_phylo_switches.cpp) when an engine is created and
// kept on the engine (mi_engine::sw).  Host code only: the launchers take the values they need
// as parameters; no kernel argument struct carries this one.
#pragma once
#include <cstddef>
#include <string>

namespace miphylo {

struct Switches {
  // gradient kernels
  bool hbm_gradient = false;   // GRADIENT_PATH=hbm: every gradient call streams its vectors through HBM
  bool walk3 = true;           // GRADIENT_WALK=v2: false (the second generation for every call)
  bool walk3_arena = true;     // WALK3_ARENA=0: arena-variant calls keep the second generation
  bool walk3_k1_lds = true;    // WALK3_K1=0: one-category LDS calls take the look-up walk only where the one-launch call applies
  int gradient_store = 0;      // GRADIENT_STORE: 0 by tree size and batch, 1 lds, 2 arena
  int walk_tile_regs = 0;      // WALK_TILE_REGS: 0 by shape, else 3 | 4
  int walk_tiles_per_wave = 0; // WALK_TILES_PER_WAVE: 0 by batch, else >= 1
  int arena_nt = -1;           // ARENA_NT: -1 by tiles per tree, 0 plain, 1 non-temporal
  bool tip_tiles = true;       // TIP_TILES=0: the kernels stage their tip bytes themselves
  bool analytic_subst = false; // SUBST_GRADIENT=analytic
  // log-likelihood kernels
  int loglik_path = 0;            // LOGLIK_PATH: 0 default, 1 valu, 2 mfma
  int loglik_evals_per_wave = 0;  // LOGLIK_EVALS_PER_WAVE: 0 by batch, else 1 | 2 | 4 | 8
  // tree set-up
  int tree_setup = 0;          // TREE_SETUP: 0 by tree size, 1 small, 2 wg, 3 lds
  int macro_slots = 0;         // MACRO_SLOTS: 0 folded into the set-up launch where it can be, 1 own, 2 seq
  int setup_records = -1;      // SETUP_RECORDS: -1 by rows of records per tree, 0 own launches, 1 quarter-waves, 2 wg
  // the one-launch call
  bool fused_setup = true;     // FUSED_SETUP=0: always the four-launch sequence
  bool fuse_finalize = true;   // FUSE_FINALIZE=0: likewise
  int fused_max_trees = 512;   // FUSED_MAX_TREES
  int fused_fence = 1;         // FUSED_FENCE: 0 none, 1 l1, 2 agent (FusedSetupArgs::fence)
  bool fused_colocate = true;  // FUSED_COLOCATE=0: set-up waves in id order
  int fused_spin_ticks = 0;    // FUSED_SPIN_MS in 100 MHz ticks (0: the launcher's default, one second)
  int fused_debug_skip = 0;    // DEBUG_FUSED_SKIP=t+1: tree t's set-up never reports (testing)
  // memory
  long long plv_bytes = -1;    // PLV_BYTES: the arena budget (-1: the engine's default)
  // placement
  bool place_table_global = false;  // PLACE_TABLE=global: the scoring gathers from memory even where the table fits LDS
  // bootstrap weights
  bool boot_hist_global = false;  // BOOT_HIST=global: the sampler's histograms are rows of the workspace even where a row fits LDS
  // split tables
  int split_hash_bits = 32;  // SPLIT_HASH_BITS: bits of the hash that choose the first slot (testing: 0 sends every split to slot 0)
  // subsplit Bayesian networks
  int sbn_trees_per_wave = 16;  // SBN_TREES_PER_WAVE: trees (lanes at work) per wave of the per-tree kernels, 16 | 32 | 64
  int gp_hybrid_z = 0;         // GP_HYBRID_Z: gridDim.z of the hybrid summand kernel (0: by the widest request, at most 16)
  bool gp_trees_global = false;  // GP_TREES_STORE=global: the per-tree kernels of the DAG's trees keep their node words in the workspace even where they fit LDS
  // 20-state kernels
  bool aa_jacobi_seq = false;        // AA_JACOBI=seq
  bool aa_post_wave = false;         // AA_POST=wave
  bool aa_pre_wave = false;          // AA_PRE=wave
  int aa_post_tiles = 0;             // AA_POST_TILES: 0 by launch size, else 1 | 2 | 4
  long aa_post_one_tile_below = -1;  // AA_POST_ONE_TILE_BELOW (-1: two workgroups per CU)
  int aa_ring = -1;                  // AA_RING: -1 by launch size, else 0 | 1 | 2 | 4
  int aa_pre_ring = -1;              // AA_PRE_RING: -1 default (1), else 0 | 1 | 2
  size_t aa_lds_pad = 0;             // AA_LDS_PAD (bytes)
};

// Fills `out` from the environment (a variable that is unset or empty keeps its default).
// A value outside a switch's accepted set leaves `error` as "NAME=value: expected ..." and
// returns false.
bool parse_switches(Switches& out, std::string& error);

}  // namespace miphylo
