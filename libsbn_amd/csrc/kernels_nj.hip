// Neighbour joining (Saitou & Nei) of a batch of distance matrices (gfx950 /
// CDNA4, wave64).  A workgroup is ONE wave and owns one matrix: the barriers below order that
// wave's own loads and stores, nothing here waits on another wave.
//
// The rule, stated so that it is reproducible.  Clusters live in slots 0..n-1; joining slots
// i < j puts the new cluster in slot i and kills slot j; slots are not compacted.  With r live
// slots and R_i = sum_k d(i, k) over the live slots in ascending order (k = i adds the 0.0 of
// the diagonal), the pair that minimises Q(i, j) = (r-2) d(i, j) - R_i - R_j is joined, the
// lowest (i, j) among equals.  delta_i = d(i, j) / 2 + (R_i - R_j) / (2 (r-2)),
// delta_j = d(i, j) - delta_i, d(u, k) = (d(i, k) + d(j, k) - d(i, j)) / 2.  The last three
// clusters a < b < c hang under the root with (d_ab + d_ac - d_bc) / 2 and its two rotations.
// Every operation is rounded once, in the order written: the file is compiled with floating-point
// contraction OFF (FLAGS_kernels_nj = -ffp-contract=off in the Makefile; a pragma does not reach
// the back end's fusion, and HIP's default would fuse (r-2) d - R_i into one
// v_fma_f64, whose single rounding can pick another pair among Q that are close), so a host
// implementation in IEEE doubles gives the same bits.  The lengths are
// clamped on their way out, never in the matrix.
//
// The joins number the internal nodes n, n+1, ... in the order they are made (a parent is made
// after its children: the ids are a post-order); renumber_tree (mi_phylo_renumber_device.h)
// then writes the tree in the reference's numbering.
//
// The working set of a matrix -- the full symmetric matrix, the row sums, the tree as joined,
// the renumbering's arrays: nj_ws_bytes -- is in LDS while it fits, else in global memory, the
// same code either way.
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_renumber_device.h"

namespace miphylo {

namespace {
using namespace dev;

__device__ __forceinline__ void nj_matrix(const NjArgs& a, int b, char* store) {
  const int lane = threadIdx.x, n = a.n;
  const int root = 2 * n - 3, R = root + 1;
  double* D = reinterpret_cast<double*>(store);  // [n][n], both halves
  double* Rs = D + (size_t)n * n;                // [n] row sums of the live slots
  double* pre_bl = Rs + n;                       // [R] lengths by the joins' node ids
  int32_t* node = reinterpret_cast<int32_t*>(pre_bl + R);  // [n] the node in a slot, -1: dead
  int32_t* pre_pid = node + n;                             // [R] parents by the joins' node ids
  int32_t* ws = pre_pid + R;                               // the renumbering's arrays
  const double* src = a.dist + (size_t)b * n * n;

  bool bad = false;
  for (int i = 0; i < n; i++)
    for (int j = lane; j < n; j += 64) {
      const double v = i == j ? 0.0 : (i < j ? src[(size_t)i * n + j] : src[(size_t)j * n + i]);
      bad = bad || !isfinite(v);
      D[(size_t)i * n + j] = v;
    }
  for (int i = lane; i < n; i += 64) node[i] = i;
  if (__any(bad)) {  // (wave-uniform)
    if (lane == 0) set_status(a.status, kBadDistance, b);
    return;
  }
  __syncthreads();

  int next = n;
  for (int r = n; r > 3; r--) {
    for (int i = lane; i < n; i += 64) {
      if (node[i] < 0) continue;
      double s = 0.0;
      for (int k = 0; k < n; k++)
        if (node[k] >= 0) s = __dadd_rn(s, D[(size_t)k * n + i]);
      Rs[i] = s;
    }
    __syncthreads();
    // the smallest Q, the lowest (i, j) among equals: a lane sees its pairs in ascending order
    const double rm2 = (double)(r - 2);
    double best_q = __builtin_inf();
    int best_i = 0x7fffffff, best_j = 0x7fffffff;
    for (int i = 0; i < n - 1; i++) {
      if (node[i] < 0) continue;  // (wave-uniform)
      const double Ri = Rs[i];
      for (int j = i + 1 + lane; j < n; j += 64) {
        if (node[j] < 0) continue;
        const double q = __dsub_rn(__dsub_rn(__dmul_rn(rm2, D[(size_t)i * n + j]), Ri), Rs[j]);
        if (q < best_q) {
          best_q = q;
          best_i = i;
          best_j = j;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double oq = __shfl_xor(best_q, off, 64);
      const int oi = __shfl_xor(best_i, off, 64), oj = __shfl_xor(best_j, off, 64);
      const bool take = oi != 0x7fffffff &&
                        (best_i == 0x7fffffff || oq < best_q || (oq == best_q && (oi < best_i || (oi == best_i && oj < best_j))));
      best_q = take ? oq : best_q;
      best_i = take ? oi : best_i;
      best_j = take ? oj : best_j;
    }
    if (best_i == 0x7fffffff) {  // (no Q compared below infinity: the distances overflowed)
      if (lane == 0) set_status(a.status, kBadDistance, b);
      return;
    }
    const int i = best_i, j = best_j;
    const double dij = D[(size_t)i * n + j];
    const double di = __dadd_rn(__ddiv_rn(dij, 2.0), __ddiv_rn(__dsub_rn(Rs[i], Rs[j]), __dmul_rn(2.0, rm2)));
    const double dj = __dsub_rn(dij, di);
    const int u = next++, ni = node[i], nj = node[j];
    __syncthreads();  // (every lane has read the pair's words)
    for (int k = lane; k < n; k += 64) {
      if (node[k] < 0 || k == i || k == j) continue;
      const double v = __ddiv_rn(__dsub_rn(__dadd_rn(D[(size_t)i * n + k], D[(size_t)j * n + k]), dij), 2.0);
      D[(size_t)i * n + k] = v;
      D[(size_t)k * n + i] = v;
    }
    if (lane == 0) {
      pre_pid[ni] = u;
      pre_pid[nj] = u;
      pre_bl[ni] = di;
      pre_bl[nj] = dj;
      node[i] = u;
      node[j] = -1;
    }
    __syncthreads();
  }
  if (lane == 0) {
    int s[3] = {0, 0, 0}, found = 0;
    for (int k = 0; k < n && found < 3; k++)
      if (node[k] >= 0) s[found++] = k;
    const double ab = D[(size_t)s[0] * n + s[1]], ac = D[(size_t)s[0] * n + s[2]], bc = D[(size_t)s[1] * n + s[2]];
    pre_bl[node[s[0]]] = __ddiv_rn(__dsub_rn(__dadd_rn(ab, ac), bc), 2.0);
    pre_bl[node[s[1]]] = __ddiv_rn(__dsub_rn(__dadd_rn(bc, ab), ac), 2.0);
    pre_bl[node[s[2]]] = __ddiv_rn(__dsub_rn(__dadd_rn(ac, bc), ab), 2.0);
    for (int q = 0; q < 3; q++) pre_pid[node[s[q]]] = root;
    pre_bl[root] = 0.0;
  }
  __syncthreads();
  for (int x = lane; x < root; x += 64) pre_bl[x] = fmin(fmax(pre_bl[x], a.tmin), a.tmax);
  __syncthreads();
  renumber_tree<false>(n, b, pre_pid, pre_bl, -1, ws, a.status, a.out_parent_ids + (size_t)b * root,
                       a.out_bl + (size_t)b * R, nullptr, nullptr);
}

__global__ __launch_bounds__(64) void nj_kernel(NjArgs a) {
  extern __shared__ __attribute__((aligned(16))) char nj_lds[];
  const int b = blockIdx.x;
  if (a.n <= kNjLdsTaxa) nj_matrix(a, b, nj_lds);
  else nj_matrix(a, b, a.ws + (size_t)b * nj_ws_bytes(a.n));
}

}  // namespace

void nj_prepare(int n) {
  if (n <= kNjLdsTaxa) allow_large_lds(reinterpret_cast<const void*>(nj_kernel), nj_ws_bytes(n));
}

void launch_nj(const NjArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  const size_t lds = a.n <= kNjLdsTaxa ? nj_ws_bytes(a.n) : 0;
  nj_prepare(a.n);
  hipLaunchKernelGGL(nj_kernel, dim3(a.B), dim3(64), lds, s, a);
}

}  // namespace miphylo
