// Quartet hybrid marginals of generalized pruning (gfx950 / CDNA4, wave64), over
// the vectors and matrices the last populate left on the device (kernels_gp.hip).
//
// A central entry e = (t,c) -> s with the lists  rootward g = (u,cu) -> t (rootsplits skipped),
// sister sigma in block(t,1-c), rotated rho in block(s,1), sorted o in block(s,0).  Per pattern
//
//   A = P(b_g)^T r(u,cu)    B = P(b_sigma) p(child_sigma)    C = P(b_e)^T (A o B)
//   D = P(b_rho) p(child_rho)    E = P(b_o) p(child_o)       l_p = sum_i C_i D_i E_i
//   summand = log(inv[g] q_sigma q_rho q_o) + sum_p w_p (log l_p - log Pr(u))
//   hybrid[e] = logsumexp of e's summands, g outermost, then sigma, rho, o innermost
//
// gp_hybrid_evolve_kernel stores Z_e = P(b_e) p(child_e) and A_e = P(b_e)^T r(t,c) once per entry
// ([G][4][Pp] with exponents, as every gp vector); gp_hybrid_summand_kernel is one wave per
// (pattern tile, formed entry, z), lane = pattern, C hoisted per (g, sigma) and C o D per
// (g, sigma, rho); the (g, sigma) pairs of an entry are dealt round-robin over blockIdx.z.  Every
// summand is formed by exactly one wave with the same operations whatever gridDim.z is.
//
// Order of summation.  Patterns: within a tile the butterfly of wave_sum, then the tiles ascending
// with one accumulator.  Summands: the maximum first, then sum exp(x - max) ascending with one
// accumulator.  A node's probability: the entries into it ascending.  No atomics.
//
// Rescaling.  Exponents are integers and add; they enter the logs as e ln 2.  A stored vector only
// has its largest entry above the threshold, so C and C o D are rescaled by the rule of
// kernels_gp.hip: no more than two scaled vectors are ever multiplied unscaled.
#include <hip/hip_runtime.h>

#include "mi_phylo_gp_device.h"

namespace miphylo {

namespace {

using namespace gpdev;

// Pr[node] (UnconditionalNodeProbabilities), its log, and inv[G] (InvertedGPCSPProbabilities) from
// the q on the device: one workgroup, the levels descending, then the leaves.
__global__ __launch_bounds__(256) void gp_node_probabilities_kernel(GpArgs a, GpHybridArgs h) {
  const int tid = threadIdx.x;
  auto visit = [&](int s) {
    double sum = 0.0;
    for (int k = a.in_range[2 * s]; k < a.in_range[2 * s + 1]; k++) {
      const int e = a.in_edges[k];
      sum += e < a.R ? a.q[e] : h.pr[a.edge[3 * e]] * a.q[e];
    }
    h.pr[s] = sum;
    h.log_pr[s] = log(sum);
  };
  for (int l = h.L - 1; l >= 0; l--) {
    const int first = h.level_range[2 * l], count = h.level_range[2 * l + 1];
    for (int k = tid; k < count; k += 256) visit(a.order[first + k]);
    __syncthreads();
  }
  for (int s = tid; s < a.n; s += 256) visit(s);
  __syncthreads();
  for (int e = tid; e < a.G; e += 256) {
    if (e < a.R) {
      h.inv[e] = 1.0;
      continue;
    }
    const double child = h.pr[a.edge[3 * e + 2]];
    h.inv[e] = child > 0.0 ? h.pr[a.edge[3 * e]] * a.q[e] / child : 0.0;
  }
}

// One lane per (entry, pattern): Z_e with the child's exponent; A_e with r's (child internal only).
__global__ __launch_bounds__(64) void gp_hybrid_evolve_kernel(GpArgs a, GpHybridArgs h) {
  const int p = blockIdx.x * kGpTile + threadIdx.x;
  const int e = a.R + blockIdx.y;
  const size_t Pp = a.Pp;
  const int t = a.edge[3 * e], c = a.edge[3 * e + 1], s = a.edge[3 * e + 2];
  const double* M = a.mats + (size_t)e * 16;
  double v[4], z[4];
  int ev;
  node_p(a, s, p, v, ev);
#pragma unroll
  for (int x = 0; x < 4; x++) z[x] = M[x * 4] * v[0] + M[x * 4 + 1] * v[1] + M[x * 4 + 2] * v[2] + M[x * 4 + 3] * v[3];
  store_vec(h.z + (size_t)e * 4 * Pp, Pp, p, z);
  h.ez[(size_t)e * Pp + p] = ev;
  if (s < a.n) return;
  const size_t i = (size_t)(t - a.n);
  double r[4], y[4];
  load_vec(a.r + (i * 2 + c) * 4 * Pp, Pp, p, r);
#pragma unroll
  for (int x = 0; x < 4; x++) y[x] = M[x] * r[0] + M[4 + x] * r[1] + M[8 + x] * r[2] + M[12 + x] * r[3];
  store_vec(h.a + (size_t)e * 4 * Pp, Pp, p, y);
  h.ea[(size_t)e * Pp + p] = a.er[(i * 2 + c) * Pp + p];
}

// One wave per (pattern tile, formed entry, z): partial[summand][tile] = the tile's sum of
// w_p (log l_p - log Pr(u)).  A lane of weight 0 contributes exactly 0, a lane with l_p = 0 -inf.
__global__ __launch_bounds__(64) void gp_hybrid_summand_kernel(GpArgs a, GpHybridArgs h) {
  const int p = blockIdx.x * kGpTile + threadIdx.x;
  const int e = h.formed[blockIdx.y];
  const size_t Pp = a.Pp;
  const double w = p < a.P ? a.weights[p] : 0.0;
  const int32_t* d = h.desc + (size_t)e * kGpHybridDesc;
  const int first = d[1], gb = d[4], sb = d[6], rb = d[8], ob = d[10];
  const int ng = d[5] - gb, ns = d[7] - sb, nr = d[9] - rb, no = d[11] - ob;
  const double* M = a.mats + (size_t)e * 16;
  for (int pair = blockIdx.z; pair < ng * ns; pair += gridDim.z) {
    const int ig = pair / ns, is = pair - ig * ns;
    const int g = a.in_edges[gb + ig], sg = sb + is;
    const double log_pr = h.log_pr[a.edge[3 * g]];
    double A[4], B[4], AB[4];
    load_vec(h.a + (size_t)g * 4 * Pp, Pp, p, A);
    load_vec(h.z + (size_t)sg * 4 * Pp, Pp, p, B);
#pragma unroll
    for (int j = 0; j < 4; j++) AB[j] = A[j] * B[j];
    Vec4 C;
#pragma unroll
    for (int y = 0; y < 4; y++) C.x[y] = M[y] * AB[0] + M[4 + y] * AB[1] + M[8 + y] * AB[2] + M[12 + y] * AB[3];
    C.e = h.ea[(size_t)g * Pp + p] + h.ez[(size_t)sg * Pp + p];
    rescale(C, a.threshold);
    for (int ir = 0; ir < nr; ir++) {
      const int rho = rb + ir;
      double D[4];
      load_vec(h.z + (size_t)rho * 4 * Pp, Pp, p, D);
      Vec4 CD;
#pragma unroll
      for (int j = 0; j < 4; j++) CD.x[j] = C.x[j] * D[j];
      CD.e = C.e + h.ez[(size_t)rho * Pp + p];
      rescale(CD, a.threshold);
      const size_t row = (size_t)first + ((size_t)(ig * ns + is) * nr + ir) * no;
      for (int io = 0; io < no; io++) {
        const int o = ob + io;
        double E[4];
        load_vec(h.z + (size_t)o * 4 * Pp, Pp, p, E);
        const double l = CD.x[0] * E[0] + CD.x[1] * E[1] + CD.x[2] * E[2] + CD.x[3] * E[3];
        const int el = CD.e + h.ez[(size_t)o * Pp + p];
        double term = 0.0;
        if (w != 0.0) term = l > 0.0 ? w * (log(l) + el * kLn2 - log_pr) : -INFINITY;
        term = wave_sum(term);
        if (threadIdx.x == 0) h.partial[(row + io) * a.tiles + blockIdx.x] = term;
      }
    }
  }
}

// One thread per summand of formed entry blockIdx.y: its tiles ascending with one accumulator, then
// the prior term.  The summand's entries follow from its index within the request (g outermost,
// o innermost) and the request's lists.
__global__ __launch_bounds__(256) void gp_hybrid_finalize_summands_kernel(GpArgs a, GpHybridArgs h, double* out_summands) {
  const int32_t* d = h.desc + (size_t)h.formed[blockIdx.y] * kGpHybridDesc;
  int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= d[2]) return;
  const size_t row = (size_t)d[1] + k;
  const int ns = d[7] - d[6], nr = d[9] - d[8], no = d[11] - d[10];
  const int o = d[10] + k % no;
  k /= no;
  const int rho = d[8] + k % nr;
  k /= nr;
  const int sg = d[6] + k % ns;
  const int g = a.in_edges[d[4] + k / ns];
  double sum = 0.0;
  for (int t = 0; t < a.tiles; t++) sum += h.partial[row * a.tiles + t];
  const double x = log(h.inv[g] * a.q[sg] * a.q[rho] * a.q[o]) + sum;
  h.summ[row] = x;
  if (out_summands) out_summands[row] = x;
}

// One thread per entry: the logsumexp of its summands in order (a -inf summand drops out; all of
// them -inf: -inf); an entry that is not fully formed gets -inf.
__global__ __launch_bounds__(256) void gp_hybrid_finalize_entries_kernel(GpArgs a, GpHybridArgs h, double* out_hybrid) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.G) return;
  const int32_t* d = h.desc + (size_t)e * kGpHybridDesc;
  double result = -INFINITY;
  if (d[0]) {
    const int first = d[1], count = d[2];
    double top = -INFINITY;
    for (int k = 0; k < count; k++) top = fmax(top, h.summ[first + k]);
    if (top > -INFINITY) {
      double sum = 0.0;
      for (int k = 0; k < count; k++) sum += exp(h.summ[first + k] - top);
      result = top + log(sum);
    }
  }
  out_hybrid[e] = result;
}

}  // namespace

void launch_gp_hybrid(const GpArgs& a, const GpHybridArgs& h, double* out_hybrid, double* out_summands, hipStream_t s) {
  hipLaunchKernelGGL(gp_node_probabilities_kernel, dim3(1), dim3(256), 0, s, a, h);
  hipLaunchKernelGGL(gp_hybrid_evolve_kernel, dim3(a.tiles, a.G - a.R), dim3(kGpTile), 0, s, a, h);
  if (h.F > 0) {
    hipLaunchKernelGGL(gp_hybrid_summand_kernel, dim3(a.tiles, h.F, h.Z), dim3(kGpTile), 0, s, a, h);
    hipLaunchKernelGGL(gp_hybrid_finalize_summands_kernel, dim3((h.widest + 255) / 256, h.F), dim3(256), 0, s, a, h, out_summands);
  }
  hipLaunchKernelGGL(gp_hybrid_finalize_entries_kernel, dim3((a.G + 255) / 256), dim3(256), 0, s, a, h, out_hybrid);
}

}  // namespace miphylo
