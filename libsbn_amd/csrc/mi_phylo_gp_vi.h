// The variational fit over the rooted trees of the subsplit DAG: what
// kernels_gp_vi.hip and mi_phylo_gp_vi.cpp share -- the arguments and the launchers.  N = 2n-1 nodes
// per rooted tree, the root N-1; blocks as mi_gp_structure gives them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace miphylo {

struct ViState;

// log_params [G] -> log q and q, normalised per block
struct GpViNormArgs {
  int n, nodes, R, G;
  const int32_t* block_range;  // [nodes][2][2]
  const double* log_params;    // [G]
  int32_t* status;
  double* out_log_q;           // [G] or null
  double* out_q;               // [G]
};
void launch_gp_vi_normalize(const GpViNormArgs& a, hipStream_t s);

// the branch lengths of T trees, drawn per entry
struct GpViSampleArgs {
  int n, T, G;
  const int32_t* entries;    // [T][N]
  const double* q_params;    // [G][2] mu, sigma
  uint64_t seed;
  int64_t first_sample;
  const ViState* vi;         // a fit's step: first_sample is the state's (else null)
  double prior_rate;
  const double* epsilon_in;  // [T][N-1] or null
  int32_t* status;
  double* out_lengths;       // [T][N] theta; 0 in the root's slot
  double* out_epsilon;       // [T][N-1]
  double* out_log_q;         // [T]
  double* out_log_prior;     // [T]
};
void launch_gp_vi_branch_sample(const GpViSampleArgs& a, hipStream_t s);

// the reparametrisation terms of every (tree, node) with the likelihood gradient gathered through new_id, and log_f
struct GpViTermsArgs {
  int n, T, G;
  const int32_t* entries;          // [T][N]
  const double* q_params;          // [G][2]
  const double* lengths;           // [T][N]
  const double* epsilon;           // [T][N-1]
  const int32_t* new_id;           // [T][N]
  const double* branch_gradient;   // [T][N] of the de-rooted trees (2n-3 edges and two more slots)
  const double *log_likelihoods, *log_prior, *log_q_branch;  // [T]
  const double* log_q_topology;    // [T] or null: 0
  const double* weights;           // [T] or null: 1
  double beta, prior_rate;
  const ViState* vi;               // a fit's step: beta is the state's (else null)
  int32_t* status;
  double* terms;                   // [T][N-1][2]: c0, c1
  double* out_log_f;               // [T]
};
void launch_gp_vi_terms(const GpViTermsArgs& a, hipStream_t s);

// The per-entry ordered sums, by ONE stable sort of (entry, position), position = t N + v: per entry the terms
// of its positions v < N-1 (terms null: skipped) and the factors of the trees that use it (factors null: skipped),
// each added in ascending position with one accumulator by the head of the entry's run; then, with factors, the
// topology gradient per block.
struct GpViSumsArgs {
  int n, T, G, nodes, R;
  const int32_t* entries;      // [T][N]
  const int32_t* block_range;  // [nodes][2][2]
  const double* terms;         // [T][N-1][2] or null
  const double* factors;       // [T] or null
  const double* q;             // [G] normalised (the topology side)
  uint32_t *keys, *keys2, *vals, *vals2;  // [T N] each
  void* sort_tmp;
  size_t sort_tmp_bytes;
  double* usage;               // [G] workspace: G_j
  double* out_q_gradient;      // [G][2] (with terms)
  double* out_gradient;        // [G] (with factors)
};
int launch_gp_vi_sums(const GpViSumsArgs& a, hipStream_t s);  // (nonzero: rocPRIM refused)

}  // namespace miphylo
