// Device helpers of generalized pruning, shared by kernels_gp.hip and
// kernels_gp_hybrid.hip: vectors with one integer exponent per pattern (true = stored x 2^e), the
// aligned sum, the rescaling rule, the butterfly over a wave and a node's p at one pattern.
#pragma once
#include <hip/hip_runtime.h>

#include "mi_phylo_kernels.h"

namespace miphylo {
namespace gpdev {

constexpr double kLn2 = 0.693147180559945309417232121458176568;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct Vec4 {
  double x[4];
  int e;
};

// acc += term, both with exponents: aligned to the larger exponent (an empty accumulator takes the term's)
__device__ __forceinline__ void add_aligned(Vec4& acc, bool& any, const double* term, int e) {
  if (!any) {
#pragma unroll
    for (int j = 0; j < 4; j++) acc.x[j] = term[j];
    acc.e = e;
    any = true;
    return;
  }
  if (e > acc.e) {
    const int d = acc.e - e;
#pragma unroll
    for (int j = 0; j < 4; j++) acc.x[j] = ldexp(acc.x[j], d) + term[j];
    acc.e = e;
  } else {
    const int d = e - acc.e;
#pragma unroll
    for (int j = 0; j < 4; j++) acc.x[j] += ldexp(term[j], d);
  }
}

__device__ __forceinline__ void rescale(Vec4& v, double threshold) {
  const double m = fmax(fmax(v.x[0], v.x[1]), fmax(v.x[2], v.x[3]));
  if (m > 0.0 && m < threshold) {
    const int k = ilogb(m);
#pragma unroll
    for (int j = 0; j < 4; j++) v.x[j] = ldexp(v.x[j], -k);
    v.e += k;
  }
}

// the tip vector of leaf `x` at pattern p
__device__ __forceinline__ void tip_vector(const GpArgs& a, int x, int p, double* out) {
  const int code = a.codes[(size_t)x * a.Cp + (p < a.P ? p : a.P - 1)];  // (a padding lane: read, never summed)
#pragma unroll
  for (int j = 0; j < 4; j++) out[j] = (code == 4 || code == j) ? 1.0 : 0.0;
}

__device__ __forceinline__ void load_vec(const double* base, size_t Pp, int p, double* out) {
#pragma unroll
  for (int j = 0; j < 4; j++) out[j] = base[(size_t)j * Pp + p];
}
__device__ __forceinline__ void store_vec(double* base, size_t Pp, int p, const double* in) {
#pragma unroll
  for (int j = 0; j < 4; j++) base[(size_t)j * Pp + p] = in[j];
}

// p(node) at pattern p with its exponent: a leaf's tip vector or the stored vector
__device__ __forceinline__ void node_p(const GpArgs& a, int node, int p, double* out, int& e) {
  if (node < a.n) {
    tip_vector(a, node, p, out);
    e = 0;
  } else {
    const size_t i = (size_t)(node - a.n);
    load_vec(a.p + i * 4 * a.Pp, a.Pp, p, out);
    e = a.ep[i * a.Pp + p];
  }
}

}  // namespace gpdev
}  // namespace miphylo
