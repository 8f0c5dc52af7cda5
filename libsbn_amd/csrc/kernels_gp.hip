// Generalized pruning over a subsplit DAG (gfx950 / CDNA4, wave64): the marginal
// likelihood over every tree of the DAG in two sweeps, and from them the per-entry likelihoods and
// the branch-length derivatives of the marginal.
//
//   phat(t,c) = sum_{e in block(t,c)} q_e P(b_e) p(child_e)       p(t) = phat(t,0) o phat(t,1)
//   rhat(s)   = [s is a rootsplit node] q_root(s) pi + sum_{e=(t,c)->s} q_e P(b_e)^T r(t,c)
//   r(t,c)    = rhat(t) o phat(t,1-c)
//   l_e       = r(t,c)^T P(b_e) p(s);  with u = V^T r, v = V^-1 p:  l_e^(k) = sum_i u_i v_i lambda_i^k e^{lambda_i b_e}
//   M         = sum_rootsplits (q_root pi) . p(root node)
//
// Patterns are independent.  A workgroup is ONE wave over a tile of kGpTile = 64 patterns and one
// node; a launch takes the nodes of one level (equal clade size), so no workgroup ever waits on
// another: the levels are ordered by the stream.  The rootward visit of a node reads each child's
// p once and writes phat_0, phat_1 and p; the leafward visit of a node reads each parent's r
// once, forms P^T r for rhat and, with p(s) at hand, the entry's l, l', l'' from the same loads,
// then writes r(s,0), r(s,1).  rhat is never stored.
//
// Order of summation.  A sum over a block's entries or over the entries into a node takes them in
// ascending entry order with one accumulator.  A sum over patterns is: within a tile the butterfly
// of wave_sum (lane l adds lane l ^ 32, then ^ 16, ... ^ 1), then the tiles in ascending order
// with one accumulator (gp_finalize_kernel).  No atomics; nothing depends on how calls are batched.
//
// Rescaling.  Every stored vector carries an integer exponent per pattern: true = stored x 2^e.
// Terms of a sum are aligned to the least-scaled term (the largest exponent) by ldexp, which is
// exact; a vector whose largest entry is below `threshold` is multiplied by the power of two that
// brings that entry into [1, 2).  So the threshold decides only where exact scalings happen.
#include <hip/hip_runtime.h>

#include "mi_phylo_gp_device.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {

using namespace gpdev;  // Vec4, add_aligned, rescale, wave_sum, node_p (mi_phylo_gp_device.h)

// One thread per entry: P(b) = I + V diag(expm1(lambda b)) V^-1 (the form of transition_kernel),
// e^{lambda_i b} and lambda_i with the one category's rate folded in.
__global__ __launch_bounds__(64) void gp_matrices_kernel(GpArgs a) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= a.G) return;
  const DevModel& m = *a.model;
  const double rate = m.cat_rate[0], b = a.b[e];
  double em[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const double l = m.lambda[i] * rate;
    em[i] = expm1(l * b);
    a.expl[(size_t)e * 8 + i] = em[i] + 1.0;
    a.expl[(size_t)e * 8 + 4 + i] = l;
  }
#pragma unroll
  for (int x = 0; x < 4; x++)
#pragma unroll
    for (int y = 0; y < 4; y++) {
      double v = x == y ? 1.0 : 0.0;
      double c = 0.0;
#pragma unroll
      for (int i = 0; i < 4; i++) c += m.V[x * 4 + i] * em[i] * m.Vinv[i * 4 + y];
      a.mats[(size_t)e * 16 + x * 4 + y] = v + c;
    }
}

// Rootward visit of internal node order[first + blockIdx.y] on pattern tile blockIdx.x.
__global__ __launch_bounds__(64) void gp_rootward_kernel(GpArgs a, int first) {
  const int p = blockIdx.x * kGpTile + threadIdx.x;
  const int t = a.order[first + blockIdx.y];
  const size_t Pp = a.Pp, i = (size_t)(t - a.n);
  Vec4 ph[2];
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const int begin = a.block_range[(t * 2 + c) * 2], end = a.block_range[(t * 2 + c) * 2 + 1];
    bool any = false;
    ph[c] = Vec4{{0.0, 0.0, 0.0, 0.0}, 0};
    for (int e = begin; e < end; e++) {
      const int child = a.edge[3 * e + 2];
      double v[4], term[4];
      int ev;
      node_p(a, child, p, v, ev);
      const double* M = a.mats + (size_t)e * 16;
      const double q = a.q[e];
#pragma unroll
      for (int x = 0; x < 4; x++)
        term[x] = q * (M[x * 4] * v[0] + M[x * 4 + 1] * v[1] + M[x * 4 + 2] * v[2] + M[x * 4 + 3] * v[3]);
      add_aligned(ph[c], any, term, ev);
    }
    rescale(ph[c], a.threshold);
    store_vec(a.phat + (i * 2 + c) * 4 * Pp, Pp, p, ph[c].x);
    a.ephat[(i * 2 + c) * Pp + p] = ph[c].e;
  }
  Vec4 pv;
#pragma unroll
  for (int j = 0; j < 4; j++) pv.x[j] = ph[0].x[j] * ph[1].x[j];
  pv.e = ph[0].e + ph[1].e;
  rescale(pv, a.threshold);
  store_vec(a.p + i * 4 * Pp, Pp, p, pv.x);
  a.ep[i * Pp + p] = pv.e;
}

// M_p and the rootsplit rows: for rootsplit entry i with node s, sum_p w_p log(pi . p(s)).
__global__ __launch_bounds__(64) void gp_marginal_kernel(GpArgs a) {
  const int p = blockIdx.x * kGpTile + threadIdx.x;
  const double w = p < a.P ? a.weights[p] : 0.0;
  const DevModel& m = *a.model;
  double M = 0.0;
  int eM = 0;
  bool any = false;
  for (int i = 0; i < a.R; i++) {
    const int s = a.edge[3 * i + 2];
    double v[4];
    int ev;
    node_p(a, s, p, v, ev);
    const double d = m.pi[0] * v[0] + m.pi[1] * v[1] + m.pi[2] * v[2] + m.pi[3] * v[3];
    const double term = w != 0.0 ? w * (log(d) + ev * kLn2) : 0.0;
    const double sum = wave_sum(term);
    if (threadIdx.x == 0) {
      double* out = a.partial + ((size_t)i * a.tiles + blockIdx.x) * kGpSums;
      out[0] = sum;
      out[1] = out[2] = out[3] = out[4] = 0.0;
    }
    if (a.matrix && p < a.P) a.matrix[(size_t)i * a.P + p] = log(d) + ev * kLn2;
    const double qd = a.q[i] * d;
    if (!any) {
      M = qd;
      eM = ev;
      any = true;
    } else if (ev > eM) {
      M = ldexp(M, eM - ev) + qd;
      eM = ev;
    } else {
      M += ldexp(qd, ev - eM);
    }
  }
  const double lm = log(M) + eM * kLn2;
  a.marg[p] = M;
  a.emarg[p] = eM;
  a.log_marg[p] = lm;
  const double sum = wave_sum(w != 0.0 ? w * lm : 0.0);
  if (threadIdx.x == 0) {
    double* out = a.partial + ((size_t)a.G * a.tiles + blockIdx.x) * kGpSums;
    out[0] = sum;
    out[1] = out[2] = out[3] = out[4] = 0.0;
  }
}

// Leafward visit of node s on one pattern tile: the entries into s in ascending order.
// kLeaf: s is a leaf (no rhat, no r).
template <bool kLeaf>
__device__ __forceinline__ void leafward_visit(const GpArgs& a, int s) {
  const int p = blockIdx.x * kGpTile + threadIdx.x;
  const size_t Pp = a.Pp;
  const DevModel& m = *a.model;
  const double w = p < a.P ? a.weights[p] : 0.0;
  double ps[4];
  int eps;
  node_p(a, s, p, ps, eps);
  double vv[4];  // V^-1 p(s)
#pragma unroll
  for (int i = 0; i < 4; i++)
    vv[i] = m.Vinv[i * 4] * ps[0] + m.Vinv[i * 4 + 1] * ps[1] + m.Vinv[i * 4 + 2] * ps[2] + m.Vinv[i * 4 + 3] * ps[3];
  const double Mp = a.marg[p];
  const int eM = a.emarg[p];
  Vec4 rh{{0.0, 0.0, 0.0, 0.0}, 0};
  bool any = false;
  const int begin = a.in_range[2 * s], end = a.in_range[2 * s + 1];
  for (int k = begin; k < end; k++) {
    const int e = a.in_edges[k];
    const double q = a.q[e];
    if (e < a.R) {  // the rootsplit entry of s: q_root pi
      if (!kLeaf) {
        double term[4];
#pragma unroll
        for (int j = 0; j < 4; j++) term[j] = q * m.pi[j];
        add_aligned(rh, any, term, 0);
      }
      continue;
    }
    const int t = a.edge[3 * e], c = a.edge[3 * e + 1];
    const size_t i = (size_t)(t - a.n);
    double r[4];
    load_vec(a.r + (i * 2 + c) * 4 * Pp, Pp, p, r);
    const int er = a.er[(i * 2 + c) * Pp + p];
    const double* Mx = a.mats + (size_t)e * 16;
    double z[4];  // P^T r
#pragma unroll
    for (int y = 0; y < 4; y++) z[y] = Mx[y] * r[0] + Mx[4 + y] * r[1] + Mx[8 + y] * r[2] + Mx[12 + y] * r[3];
    if (!kLeaf) {
      double term[4];
#pragma unroll
      for (int j = 0; j < 4; j++) term[j] = q * z[j];
      add_aligned(rh, any, term, er);
    }
    // the entry's likelihood and its derivatives, exponent er + eps
    const double l0 = z[0] * ps[0] + z[1] * ps[1] + z[2] * ps[2] + z[3] * ps[3];
    double l1 = 0.0, l2 = 0.0;
    const double* ex = a.expl + (size_t)e * 8;
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const double u = m.V[x] * r[0] + m.V[4 + x] * r[1] + m.V[8 + x] * r[2] + m.V[12 + x] * r[3];
      const double uve = u * vv[x] * ex[x], lam = ex[4 + x];
      l1 += lam * uve;
      l2 += lam * lam * uve;
    }
    const int el = er + eps;
    const double logl = log(l0) + el * kLn2;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
    if (w != 0.0) {
      const double d1 = ldexp(q * l1 / Mp, el - eM), d2 = ldexp(q * l2 / Mp, el - eM);
      t0 = w * logl;
      t1 = w * (l1 / l0);
      t2 = w * d1;
      t3 = w * (d2 - d1 * d1);
      t4 = w * (d1 * d1);
    }
    t0 = wave_sum(t0);
    t1 = wave_sum(t1);
    t2 = wave_sum(t2);
    t3 = wave_sum(t3);
    t4 = wave_sum(t4);
    if (threadIdx.x == 0) {
      double* out = a.partial + ((size_t)e * a.tiles + blockIdx.x) * kGpSums;
      out[0] = t0;
      out[1] = t1;
      out[2] = t2;
      out[3] = t3;
      out[4] = t4;
    }
    if (a.matrix && p < a.P) a.matrix[(size_t)e * a.P + p] = logl;
  }
  if (kLeaf) return;
  const size_t i = (size_t)(s - a.n);
#pragma unroll
  for (int c = 0; c < 2; c++) {
    double o[4];
    load_vec(a.phat + (i * 2 + (1 - c)) * 4 * Pp, Pp, p, o);
    Vec4 rv;
#pragma unroll
    for (int j = 0; j < 4; j++) rv.x[j] = rh.x[j] * o[j];
    rv.e = rh.e + a.ephat[(i * 2 + (1 - c)) * Pp + p];
    rescale(rv, a.threshold);
    store_vec(a.r + (i * 2 + c) * 4 * Pp, Pp, p, rv.x);
    a.er[(i * 2 + c) * Pp + p] = rv.e;
  }
}

__global__ __launch_bounds__(64) void gp_leafward_kernel(GpArgs a, int first) {
  leafward_visit<false>(a, a.order[first + blockIdx.y]);
}
__global__ __launch_bounds__(64) void gp_leaves_kernel(GpArgs a) { leafward_visit<true>(a, blockIdx.y); }

// the tiles of every row in ascending order, one accumulator
__global__ __launch_bounds__(256) void gp_finalize_kernel(GpArgs a) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((size_t)a.G + 1) * kGpSums) return;
  const size_t row = idx / kGpSums, k = idx % kGpSums;
  double sum = 0.0;
  for (int t = 0; t < a.tiles; t++) sum += a.partial[(row * a.tiles + t) * kGpSums + k];
  a.sums[idx] = sum;
}

__global__ __launch_bounds__(256) void gp_outputs_kernel(GpArgs a, double* per_gpcsp, double* log_marginal,
                                                         double* ll_deriv, double* g, double* h, double* s_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0 && log_marginal) *log_marginal = a.sums[(size_t)a.G * kGpSums];
  if (e >= a.G) return;
  const double* row = a.sums + (size_t)e * kGpSums;
  if (per_gpcsp) per_gpcsp[e] = row[0];
  if (ll_deriv) {
    ll_deriv[2 * e] = row[0];
    ll_deriv[2 * e + 1] = row[1];
  }
  if (g) g[e] = row[2];
  if (h) h[e] = row[3];
  if (s_out) s_out[e] = row[4];
}

}  // namespace

void launch_gp_matrices(const GpArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gp_matrices_kernel, dim3((a.G + 63) / 64), dim3(64), 0, s, a);
}
void launch_gp_rootward(const GpArgs& a, int first, int count, hipStream_t s) {
  hipLaunchKernelGGL(gp_rootward_kernel, dim3(a.tiles, count), dim3(kGpTile), 0, s, a, first);
}
void launch_gp_marginal(const GpArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gp_marginal_kernel, dim3(a.tiles), dim3(kGpTile), 0, s, a);
}
void launch_gp_leafward(const GpArgs& a, int first, int count, hipStream_t s) {
  hipLaunchKernelGGL(gp_leafward_kernel, dim3(a.tiles, count), dim3(kGpTile), 0, s, a, first);
}
void launch_gp_leaves(const GpArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gp_leaves_kernel, dim3(a.tiles, a.n), dim3(kGpTile), 0, s, a);
}
void launch_gp_finalize(const GpArgs& a, hipStream_t s) {
  const size_t total = ((size_t)a.G + 1) * kGpSums;
  hipLaunchKernelGGL(gp_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
}
void launch_gp_outputs(const GpArgs& a, double* per_gpcsp, double* log_marginal, double* ll_deriv, double* g, double* h,
                       double* s_out, hipStream_t s) {
  hipLaunchKernelGGL(gp_outputs_kernel, dim3((a.G + 255) / 256), dim3(256), 0, s, a, per_gpcsp, log_marginal, ll_deriv,
                     g, h, s_out);
}

}  // namespace miphylo
