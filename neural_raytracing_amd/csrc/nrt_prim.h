// nrt_prim.h -- RoundBoxSDF and CapsuleSDF (sdfs.py:46-86): the per-primitive expressions, their
// gradients and parameter gradients, shared by the march kernels (nrt_kernels.h sdf_value /
// sdf_gradient, nrt_prim.hip) and the training kernels (nrt_prim.hip).
//
// Both are a smooth-min (utils.py:386-387, k = 16) over n primitives and have no residual MLP:
//   v(p) = -log(max(sum_i exp(-k sd_i), 1e-4)) / k
//   box      (sdfs.py:61-68): u = (I + tfs_i) p - c_i, q = |u| - b_i,
//            sd_i = |max(q, 1e-7)|_2 + min(max(q_x, q_y, q_z), -1e-7)
//   capsule  (sdfs.py:78-86): pa = p - a_i, ba = b_i - a_i, h = (pa . ba) / clamp(ba . ba, 0, 1),
//            sd_i = |pa - ba h| - r_i     (h is not clamped: an infinite cylinder, as the reference)
// RoundBoxSDF.radii is a parameter its forward never reads; it is not packed.
//
// Packed table, 16 floats a primitive (nrt_sdf_create_round_boxes / _capsules):
//   box      [0..8] I + tfs row-major, [9..11] c, [12..14] b, [15] 0
//   capsule  [0..2] a, [3..5] ba, [6] den = clamp(ba . ba, 0, 1), [7] r,
//            [8] 1 where the clamp passes ba . ba's gradient (ba . ba <= 1) else 0, [9..15] 0
//
// Every function has one fixed statement order and spells its fused multiply-adds out, so a
// point's bits do not depend on which kernel evaluates it (the schedule / precision invariance
// the tests hold with torch.equal).  TP is the table pointer type: constant address space,
// LDS or plain.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace nrt {
namespace prim {

constexpr int kBox = 3, kCapsule = 4;  // SdfDev::kind, NRT_PRIM_ROUND_BOX / NRT_PRIM_CAPSULE
constexpr int kPrimF = 16;             // floats a packed primitive
constexpr int kMaxPrims = 1024;        // table limit (64 KB: fits the LDS copy of every kernel)
constexpr float kClampLo = 1e-7f;      // sdfs.py:64, 66
constexpr float kSumMin = 1e-4f;       // smooth_min's clamp (utils.py:387)

__host__ __device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// ---- packing (host creation and the device refresh run the same statements) -------------------
// box: A = centers [n,3], B = b [n,3], C = tfs [n,3,3]; capsule: A = a [n,3], B = b [n,3], C = radii [n]
template <int KIND>
__host__ __device__ __forceinline__ void pack(const float* A, const float* B, const float* C, int i,
                                              float* d) {
  if (KIND == kBox) {
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) d[3 * a + b] = C[(size_t)i * 9 + 3 * a + b] + (a == b ? 1.f : 0.f);
    for (int a = 0; a < 3; ++a) { d[9 + a] = A[i * 3 + a]; d[12 + a] = B[i * 3 + a]; }
    d[15] = 0.f;
  } else {
    const float b0 = B[i * 3] - A[i * 3], b1 = B[i * 3 + 1] - A[i * 3 + 1], b2 = B[i * 3 + 2] - A[i * 3 + 2];
    const float bb = fmaf(b2, b2, fmaf(b1, b1, b0 * b0));
    d[0] = A[i * 3]; d[1] = A[i * 3 + 1]; d[2] = A[i * 3 + 2];
    d[3] = b0; d[4] = b1; d[5] = b2;
    d[6] = fminf(fmaxf(bb, 0.f), 1.f);  // .clamp(min=0, max=1) binds to the denominator (sdfs.py:82-83)
    d[7] = C[i];
    d[8] = (bb >= 0.f && bb <= 1.f) ? 1.f : 0.f;
    for (int a = 9; a < 16; ++a) d[a] = 0.f;
  }
}

// ---- one primitive: signed distance, and its gradient n = d sd / d p ---------------------------
struct BoxTerm {
  float u[3], q[3], m[3], up, sd;
  int arg;    // the component torch.maximum(x, maximum(y, z)) takes (x on x >= max(y, z), then y on y >= z)
  bool down;  // max q <= -1e-7: the clamp(max=-1e-7) passes its gradient
};
template <class TP>
__host__ __device__ __forceinline__ BoxTerm box_term(TP s, float x, float y, float z) {
  BoxTerm t;
  t.u[0] = fmaf(s[2], z, fmaf(s[1], y, s[0] * x)) - s[9];
  t.u[1] = fmaf(s[5], z, fmaf(s[4], y, s[3] * x)) - s[10];
  t.u[2] = fmaf(s[8], z, fmaf(s[7], y, s[6] * x)) - s[11];
  t.q[0] = fabsf(t.u[0]) - s[12];
  t.q[1] = fabsf(t.u[1]) - s[13];
  t.q[2] = fabsf(t.u[2]) - s[14];
  t.m[0] = fmaxf(t.q[0], kClampLo);
  t.m[1] = fmaxf(t.q[1], kClampLo);
  t.m[2] = fmaxf(t.q[2], kClampLo);
  t.up = sqrtf(fmaf(t.m[2], t.m[2], fmaf(t.m[1], t.m[1], t.m[0] * t.m[0])));
  const float yz = fmaxf(t.q[1], t.q[2]);
  const float mq = fmaxf(t.q[0], yz);
  t.arg = t.q[0] >= yz ? 0 : (t.q[1] >= t.q[2] ? 1 : 2);
  t.down = mq <= -kClampLo;
  t.sd = t.up + fminf(mq, -kClampLo);
  return t;
}
// e = d sd / d q (torch's clamp passes the gradient on q >= 1e-7; up >= 1e-7 sqrt(3) > 0)
__host__ __device__ __forceinline__ void box_dq(const BoxTerm& t, float e[3]) {
  const float iu = 1.f / t.up;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    e[a] = (t.q[a] >= kClampLo ? t.m[a] * iu : 0.f) + ((t.down && t.arg == a) ? 1.f : 0.f);
}

struct CapTerm {
  float pa[3], v[3], h, r, sd;
};
template <class TP>
__host__ __device__ __forceinline__ CapTerm cap_term(TP s, float x, float y, float z) {
  CapTerm t;
  t.pa[0] = x - s[0]; t.pa[1] = y - s[1]; t.pa[2] = z - s[2];
  t.h = fmaf(t.pa[2], s[5], fmaf(t.pa[1], s[4], t.pa[0] * s[3])) / s[6];
  t.v[0] = fmaf(-t.h, s[3], t.pa[0]);
  t.v[1] = fmaf(-t.h, s[4], t.pa[1]);
  t.v[2] = fmaf(-t.h, s[5], t.pa[2]);
  t.r = sqrtf(fmaf(t.v[2], t.v[2], fmaf(t.v[1], t.v[1], t.v[0] * t.v[0])));
  t.sd = t.r - s[7];
  return t;
}

// sd_i of primitive s at (x, y, z)
template <int KIND, class TP>
__host__ __device__ __forceinline__ float prim_sd(TP s, float x, float y, float z) {
  if (KIND == kBox) return box_term(s, x, y, z).sd;
  return cap_term(s, x, y, z).sd;
}

// sd_i and n = d sd_i / d p
template <int KIND, class TP>
__host__ __device__ __forceinline__ float prim_sd_n(TP s, float x, float y, float z, float n[3]) {
  if (KIND == kBox) {
    const BoxTerm t = box_term(s, x, y, z);
    float e[3];
    box_dq(t, e);
    const float f0 = sgn(t.u[0]) * e[0], f1 = sgn(t.u[1]) * e[1], f2 = sgn(t.u[2]) * e[2];
    n[0] = fmaf(s[6], f2, fmaf(s[3], f1, s[0] * f0));  // (I + tfs)^T f
    n[1] = fmaf(s[7], f2, fmaf(s[4], f1, s[1] * f0));
    n[2] = fmaf(s[8], f2, fmaf(s[5], f1, s[2] * f0));
    return t.sd;
  }
  const CapTerm t = cap_term(s, x, y, z);
  // u = v / |v| (torch's norm has a zero gradient at 0); n = u - ba (u . ba) / den
  const float ir = t.r > 0.f ? 1.f / t.r : 0.f;
  const float u0 = t.v[0] * ir, u1 = t.v[1] * ir, u2 = t.v[2] * ir;
  const float ubd = fmaf(u2, s[5], fmaf(u1, s[4], u0 * s[3])) / s[6];
  n[0] = fmaf(-ubd, s[3], u0);
  n[1] = fmaf(-ubd, s[4], u1);
  n[2] = fmaf(-ubd, s[5], u2);
  return t.sd;
}

// ---- the smooth-min over a table ------------------------------------------------------------
template <int KIND, class TP>
__host__ __device__ __forceinline__ float table_value(TP tab, int n, float k, float x, float y, float z) {
  float acc = 0.f;
  for (int i = 0; i < n; ++i, tab += kPrimF) acc += expf(-k * prim_sd<KIND>(tab, x, y, z));
  return -logf(fmaxf(acc, kSumMin)) / k;
}

// g = d v / d p = (1 / S) sum_i w_i n_i; exactly zero where the 1e-4 clamp is active.  Returns S.
template <int KIND, class TP>
__host__ __device__ __forceinline__ float table_grad(TP tab, int n, float k, float x, float y, float z,
                                                     float g[3]) {
  float acc = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
  for (int i = 0; i < n; ++i, tab += kPrimF) {
    float nn[3];
    const float w = expf(-k * prim_sd_n<KIND>(tab, x, y, z, nn));
    acc += w;
    g0 = fmaf(w, nn[0], g0);
    g1 = fmaf(w, nn[1], g1);
    g2 = fmaf(w, nn[2], g2);
  }
  const float sc = acc >= kSumMin ? 1.f / acc : 0.f;
  g[0] = g0 * sc; g[1] = g1 * sc; g[2] = g2 * sc;
  return acc;
}

// ---- parameter gradients of J = sum_points (dv v + dg . g) ----------------------------------
// With alpha_i = w_i / S, n_i = d sd_i / d p, beta_i = dg . n_i, gamma = sum_j alpha_j beta_j,
// kappa_i = -k alpha_i (beta_i - gamma), c_i = dv alpha_i + kappa_i:
//   dJ / d theta_i = c_i d sd_i / d theta_i + alpha_i d beta_i / d theta_i   (p, dg held fixed)
// -- the second term is the double backward of the create_graph=True normal (sdfs.py:184-197).
//
// box, with s = sign(u), e = d sd / d q, f = s e, M = (I + tfs) dg, w = M s and, inside one smooth
// piece, h_b = d beta / d q_b = A_b (w_b - m_b (sum_a A_a w_a m_a) / up^2) / up  (A_a = [q_a >= 1e-7]):
//   E = c f + alpha s h;  dc = -E;  db = -(c e + alpha h);  dtfs = E p^T + alpha f dg^T
// fields: [0..8] dtfs, [9..11] dc, [12..14] db
//
// capsule, with u = v / r, ub = u . ba, gb = dg . ba, cl = [ba . ba <= 1], in the variables
// (pa, ba) -- d/da = -d/dpa - d/dba, d/db = d/dba:
//   G_pa = u - (ub / den) ba   (= n)
//   G_ba = -h u - (ub / den) pa + (2 cl h ub / den) ba
//   wv = (dg - (dg . u) u) / r,  y = (ba - ub u) / r,  z = wv - (gb / den) y,  zb = z . ba
//   B_pa = z - (zb / den) ba
//   B_ba = -h z - (zb / den) pa + (2 cl h zb / den) ba - (gb / den) u - (ub / den) dg
//          + (2 cl ub gb / den^2) ba
//   da = -(c (G_pa + G_ba) + alpha (B_pa + B_ba));  db = c G_ba + alpha B_ba;  dr = -c
// fields: [0..2] da, [3..5] db, [6] dr
template <int KIND>
struct Fields {
  static constexpr int N = KIND == kBox ? 15 : 7;
};

// beta_i = dg . n_i needs only n_i: prim_sd_n.  accumulate(): one point's contribution to the
// fields of primitive s; inv_S = 1 / S (the caller skips clamped points), gamma as above.
template <int KIND, class TP>
__host__ __device__ __forceinline__ void accumulate(TP s, float x, float y, float z, float k,
                                                    float inv_S, float gamma, float dv,
                                                    bool has_dg, const float dg[3], float* acc) {
  if (KIND == kBox) {
    const BoxTerm t = box_term(s, x, y, z);
    const float alpha = expf(-k * t.sd) * inv_S;
    float e[3], sg[3], f[3], h[3] = {0.f, 0.f, 0.f};
    box_dq(t, e);
#pragma unroll
    for (int a = 0; a < 3; ++a) { sg[a] = sgn(t.u[a]); f[a] = sg[a] * e[a]; }
    float beta = 0.f;
    if (has_dg) {
      float w[3];
      w[0] = fmaf(s[2], dg[2], fmaf(s[1], dg[1], s[0] * dg[0])) * sg[0];
      w[1] = fmaf(s[5], dg[2], fmaf(s[4], dg[1], s[3] * dg[0])) * sg[1];
      w[2] = fmaf(s[8], dg[2], fmaf(s[7], dg[1], s[6] * dg[0])) * sg[2];
      beta = fmaf(w[2], e[2], fmaf(w[1], e[1], w[0] * e[0]));
      const float iu = 1.f / t.up;
      float wm = 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a)
        if (t.q[a] >= kClampLo) wm = fmaf(w[a], t.m[a], wm);
      wm = wm * iu * iu;
#pragma unroll
      for (int a = 0; a < 3; ++a)
        if (t.q[a] >= kClampLo) h[a] = (w[a] - t.m[a] * wm) * iu;
    }
    const float c = fmaf(dv, alpha, -k * alpha * (beta - gamma));
    const float pp[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float E = fmaf(c, f[a], alpha * sg[a] * h[a]);
#pragma unroll
      for (int b = 0; b < 3; ++b)
        acc[3 * a + b] += fmaf(E, pp[b], has_dg ? alpha * f[a] * dg[b] : 0.f);
      acc[9 + a] -= E;
      acc[12 + a] -= fmaf(c, e[a], alpha * h[a]);
    }
    return;
  }
  const CapTerm t = cap_term(s, x, y, z);
  const float alpha = expf(-k * t.sd) * inv_S;
  const float ba[3] = {s[3], s[4], s[5]};
  const float iden = 1.f / s[6], cl2 = 2.f * s[8];
  const float ir = t.r > 0.f ? 1.f / t.r : 0.f;
  float u[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) u[a] = t.v[a] * ir;
  const float ub = fmaf(u[2], ba[2], fmaf(u[1], ba[1], u[0] * ba[0]));
  const float ubd = ub * iden;
  float Gpa[3], Gba[3], Bpa[3] = {0.f, 0.f, 0.f}, Bba[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    Gpa[a] = fmaf(-ubd, ba[a], u[a]);
    Gba[a] = fmaf(cl2 * t.h * ubd, ba[a], fmaf(-ubd, t.pa[a], -t.h * u[a]));
  }
  float beta = 0.f;
  if (has_dg) {
    beta = fmaf(dg[2], Gpa[2], fmaf(dg[1], Gpa[1], dg[0] * Gpa[0]));
    const float gu = fmaf(dg[2], u[2], fmaf(dg[1], u[1], dg[0] * u[0]));
    const float gbd = fmaf(dg[2], ba[2], fmaf(dg[1], ba[1], dg[0] * ba[0])) * iden;
    float zv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float wv = (dg[a] - gu * u[a]) * ir;
      const float yv = (ba[a] - ub * u[a]) * ir;
      zv[a] = fmaf(-gbd, yv, wv);
    }
    const float zbd = fmaf(zv[2], ba[2], fmaf(zv[1], ba[1], zv[0] * ba[0])) * iden;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      Bpa[a] = fmaf(-zbd, ba[a], zv[a]);
      Bba[a] = -t.h * zv[a] - zbd * t.pa[a] + (cl2 * t.h * zbd) * ba[a] - gbd * u[a] - ubd * dg[a] +
               (cl2 * ubd * gbd) * ba[a];
    }
  }
  const float c = fmaf(dv, alpha, -k * alpha * (beta - gamma));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float db = fmaf(c, Gba[a], alpha * Bba[a]);
    acc[a] -= fmaf(c, Gpa[a], alpha * Bpa[a]) + db;
    acc[3 + a] += db;
  }
  acc[6] -= c;
}

}  // namespace prim
}  // namespace nrt
