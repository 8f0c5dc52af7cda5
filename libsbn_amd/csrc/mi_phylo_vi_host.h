// The fit object on the host: struct mi_vi and what mi_phylo_vi.cpp (the
// unrooted fit, and every mi_vi_* call) and mi_phylo_gp_vi.cpp (the fit over the rooted trees of a
// subsplit DAG) share.  Host code only.
#pragma once
#include <string>

#include "mi_phylo_engine.h"

struct mi_gp;

// Everything a fit holds on the device is one block (`pool`), cut at creation.
struct mi_vi {
  mi_engine* e = nullptr;
  mi_vi_options o{};
  int n = 0, E = 0, T0 = 0, K = 0, R = 0, S = 0, C = 0, parents = 0, P = 0, V = 0, pc = 0, blocks = 0;
  Buffer pool;
  std::string grad_path;
  // the state
  ViState* state = nullptr;
  double *phi = nullptr, *q = nullptr, *m_sbn = nullptr, *v_sbn = nullptr, *m_q = nullptr, *v_q = nullptr;
  // the support's tables
  int32_t *d_range = nullptr, *d_desc = nullptr, *d_psp = nullptr;
  double* params = nullptr;  // [K][param_count]
  // a step's buffers: the support trees with the samples behind them, and what the calls hand on
  int32_t *all_pid = nullptr, *root = nullptr, *slot = nullptr, *counts = nullptr, *clades = nullptr,
          *prange = nullptr, *pparent = nullptr, *edge = nullptr, *sparams = nullptr, *index = nullptr;
  uint32_t* bits = nullptr;
  double *lp = nullptr, *bl = nullptr, *eps = nullptr, *lqb = nullptr, *lprior = nullptr, *ll = nullptr, *g = nullptr,
         *rooting = nullptr, *lqt = nullptr, *qgrad = nullptr, *f = nullptr, *grad = nullptr, *factors = nullptr,
         *glq = nullptr;
  // the optimiser
  int32_t* block_flags = nullptr;
  double* trace = nullptr;
  // A fit over the rooted trees of a subsplit DAG (mi_gp_vi_create): `gp` is set, T0 is 0,
  // P = V = G, and of the arrays above a step uses all_pid, edge, bl, eps, lqb, lprior, ll, g, lqt, qgrad, f,
  // grad and factors for the de-rooted particles.  What it adds: the rooted particles, the normalised table,
  // the map from rooted node to unrooted edge, and the workspace of the ordered sums.
  mi_gp* gp = nullptr;
  int32_t *r_parents = nullptr, *r_entries = nullptr, *new_id = nullptr;  // [K][2n-2], [K][2n-1] twice
  double *r_lengths = nullptr, *log_q = nullptr, *qn = nullptr, *usage = nullptr, *sums = nullptr, *terms = nullptr;
  uint32_t *keys = nullptr, *keys2 = nullptr, *vals = nullptr, *vals2 = nullptr;
  char* sort_tmp = nullptr;
  size_t sort_bytes = 0;
};

// mi_phylo_vi.cpp: the last three launches of a step (check, apply, finish) from device arrays
int vi_enqueue_update(mi_vi* v, hipStream_t s, const double* g_sbn, const double* g_q, const double* ll, const double* lprior,
                      const double* lqt, const double* lqb, double* out_row);
int vi_check_options(const mi_vi_options& o);
// mi_phylo_gp_vi.cpp: one step of a DAG fit as one chain of launches, and its line for mi_engine_last_call_path
int gp_vi_enqueue_step(mi_vi* v, hipStream_t s);
std::string gp_vi_path(const mi_vi* v, int steps);
