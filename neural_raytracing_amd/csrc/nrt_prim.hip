// nrt_prim.hip -- RoundBoxSDF and CapsuleSDF (sdfs.py:46-86) on the HIP path: SDF handles over a
// packed primitive table, lane-per-ray march kernels for these MLP-free kinds, and the fused
// training kernels of their smooth-min.  The expressions live in nrt_prim.h.
//
//   k_prim_eval        sdf(p) on a flat batch                       sdfs.py:61-68, 78-86
//   k_prim_intersect   sphere trace + 128-step coarse scan          sdfs.py:111-137, 232-249
//   k_prim_normals     raw gradient, unit normal, p += 5 eps n      sdfs.py:152-158, 184-197
//   k_prim_occlusion   shadow-ray march                             sdfs.py:162-181
//   k_prim_sm_fwd / _pre / _bwd / _reduce   value, gradient and parameter gradients (training)
//
// The per-wave kernels (k_intersect, k_occlusion, k_sdf_grad) evaluate 32 rays on 64 lanes and carve
// per-wave LDS slabs for an MLP; without matrix work both buy nothing.  Here every lane owns a ray
// or point, the loop over the primitives is wave-uniform, and the table is read either through the
// constant address space (scalar loads, LDS = false) or from an LDS copy staged once per block
// (LDS = true, option "prim_march" = 2).  Same device functions as the per-wave kernels, so the same
// bits.
#include "nrt_launch.h"

#include <vector>

namespace nrt {
namespace {

constexpr int kPrimBlock = 256;

// the table of this launch: the SDF's (constant address space) or the block's LDS copy
template <bool LDS>
__device__ __forceinline__ void stage_table(const SdfDev& s, float* ls) {
  if (LDS) {
    const int nf = s.n_spheres * prim::kPrimF;
    for (int q = threadIdx.x; q < nf; q += blockDim.x) ls[q] = s.spheres[q];
    __syncthreads();
  }
}

template <int KIND, bool LDS>
__device__ __forceinline__ float value_at(const SdfDev& s, const float* ls, float x, float y, float z) {
  if constexpr (LDS) return prim::table_value<KIND>(ls, s.n_spheres, s.k, x, y, z);
  else return prim::table_value<KIND>((const ConstF*)s.spheres, s.n_spheres, s.k, x, y, z);
}

template <int KIND, bool LDS>
__device__ __forceinline__ void grad_at(const SdfDev& s, const float* ls, float x, float y, float z,
                                        float g[3]) {
  if constexpr (LDS) prim::table_grad<KIND>(ls, s.n_spheres, s.k, x, y, z, g);
  else prim::table_grad<KIND>((const ConstF*)s.spheres, s.n_spheres, s.k, x, y, z, g);
}

template <int KIND, bool LDS>
__global__ void __launch_bounds__(kPrimBlock) k_prim_eval(const SdfDev* __restrict__ sp,
                                                          const float* __restrict__ p, int64_t M,
                                                          float* __restrict__ out) {
  extern __shared__ float ls[];
  const SdfDev s = *sp;
  stage_table<LDS>(s, ls);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  out[i] = value_at<KIND, LDS>(s, ls, p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
}

// k_intersect's contract (nrt_kernels.h) with one ray per lane: the same rounding recipe of the
// query points, the wave leaves the march when none of its rays is live, 1 + 128 + 1 scan
// evaluations when primary, scan_idx, per-group scan steps, the evals counter, the wave-aggregated
// hit list, n and raw_n zeroed.
template <int KIND, bool LDS>
__global__ void __launch_bounds__(kPrimBlock) k_prim_intersect(
    const SdfDev* __restrict__ sp, const float* __restrict__ rays, int64_t P, MarchArgs a,
    float* __restrict__ t_out, uint8_t* __restrict__ hit_out, float* __restrict__ p_out,
    float* __restrict__ n_out, float* __restrict__ rawn_out, float* __restrict__ thr_out,
    int32_t* __restrict__ hit_idx, int32_t* __restrict__ hit_count) {
  extern __shared__ float ls[];
  const SdfDev s = *sp;
  stage_table<LDS>(s, ls);
  const int lane = lane_id();
  const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = ray < P;
  if (!wave_any(valid)) return;  // whole wave past the batch
  const int64_t rr = valid ? ray : P - 1;
  const float ox = rays[rr * 6], oy = rays[rr * 6 + 1], oz = rays[rr * 6 + 2];
  const float dx = rays[rr * 6 + 3], dy = rays[rr * 6 + 4], dz = rays[rr * 6 + 5];
  unsigned long long nev = 0;  // wave-uniform: ray-evaluations executed for live rays

  // sphere tracing (sdfs.py:119-131): a ray that stopped marching never changes again
  float t = 0.f;
  bool live = valid, hit = false;
  for (int i = 0; i < a.max_steps; ++i) {
    live = live && (t < a.max_t);
    const uint64_t lm = __ballot(live);
    if (lm == 0ull) break;
    nev += (unsigned long long)__popcll(lm);
    const float px = __fadd_rn(ox, __fmul_rn(dx, t));
    const float py = __fadd_rn(oy, __fmul_rn(dy, t));
    const float pz = __fadd_rn(oz, __fmul_rn(dz, t));
    const float d = value_at<KIND, LDS>(s, ls, px, py, pz);
    const bool now = live && (d <= a.eps);
    hit = hit || now;
    live = live && !now;
    if (live) t = t + d;
  }

  // coarse scan (sdfs.py:238-249): sdf(o), 128 samples at fl32(step (j + 1)), then sdf(best_pos)
  float thr = 0.f;
  int idx = 0;
  if (a.primary) {
    const double step = scan_step_of(a, rr);
    float best = value_at<KIND, LDS>(s, ls, ox, oy, oz);
    for (int j = 0; j < 128; ++j) {
      const float ts = (float)(step * (double)(j + 1));
      const float d = value_at<KIND, LDS>(s, ls, __fadd_rn(ox, __fmul_rn(ts, dx)),
                                          __fadd_rn(oy, __fmul_rn(ts, dy)),
                                          __fadd_rn(oz, __fmul_rn(ts, dz)));
      if (d < best) idx = j + 1;
      best = fminf(best, d);
    }
    const float tb = __fmul_rn((float)idx, (float)step);
    thr = -1000.f * value_at<KIND, LDS>(s, ls, __fadd_rn(ox, __fmul_rn(tb, dx)),
                                        __fadd_rn(oy, __fmul_rn(tb, dy)),
                                        __fadd_rn(oz, __fmul_rn(tb, dz)));
    nev += 130ull * (unsigned long long)__popcll(__ballot(valid));
  }
  if (a.evals && lane == 0) atomicAdd(a.evals, nev);

  if (valid) {
    t_out[ray] = t;
    hit_out[ray] = hit ? 1 : 0;
    p_out[ray * 3] = __fadd_rn(ox, __fmul_rn(t, dx));
    p_out[ray * 3 + 1] = __fadd_rn(oy, __fmul_rn(t, dy));
    p_out[ray * 3 + 2] = __fadd_rn(oz, __fmul_rn(t, dz));
    n_out[ray * 3] = 0.f; n_out[ray * 3 + 1] = 0.f; n_out[ray * 3 + 2] = 0.f;
    if (rawn_out) { rawn_out[ray * 3] = 0.f; rawn_out[ray * 3 + 1] = 0.f; rawn_out[ray * 3 + 2] = 0.f; }
    if (a.primary) thr_out[ray] = thr;
    if (a.primary && a.scan_idx) a.scan_idx[ray] = idx;
  }
  if (hit_idx) {
    // wave-aggregated append of the hit rays (order is irrelevant downstream)
    const uint64_t m = __ballot(valid && hit);
    const int cnt = __popcll(m);
    int base = 0;
    if (lane == 0 && cnt) base = atomicAdd(hit_count, cnt);
    base = __shfl(base, 0);
    if (valid && hit) {
      const int off = __popcll(m & ((1ull << lane) - 1ull));
      hit_idx[base + off] = (int32_t)ray;
    }
  }
}

// k_sdf_grad's contract with one point per lane (grid-stride; a device-side count bounds the list)
template <int KIND, bool LDS>
__global__ void __launch_bounds__(kPrimBlock) k_prim_normals(
    const SdfDev* __restrict__ sp, const float* __restrict__ p, const int32_t* __restrict__ index,
    const int32_t* __restrict__ count, int64_t M, float* __restrict__ grad,
    float* __restrict__ n_out, float* __restrict__ p_io, float offset_eps) {
  extern __shared__ float ls[];
  const SdfDev s = *sp;
  stage_table<LDS>(s, ls);
  int64_t total = count ? (int64_t)(*count) : M;
  if (total > M) total = M;
  const float* pp = p_io ? p_io : p;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t idx = index ? (int64_t)index[i] : i;
    const float x = pp[idx * 3], y = pp[idx * 3 + 1], z = pp[idx * 3 + 2];
    float g[3];
    grad_at<KIND, LDS>(s, ls, x, y, z, g);
    if (grad) { grad[idx * 3] = g[0]; grad[idx * 3 + 1] = g[1]; grad[idx * 3 + 2] = g[2]; }
    if (n_out) {
      // normals[hit] = normalize(raw, eps=1e-6); p[hit] += normals * eps * 5  (sdfs.py:156-157)
      float nx = g[0], ny = g[1], nz = g[2];
      normalize3(nx, ny, nz, 1e-6f);
      n_out[idx * 3] = nx; n_out[idx * 3 + 1] = ny; n_out[idx * 3 + 2] = nz;
      if (p_io) {
        p_io[idx * 3] = x + (nx * offset_eps) * 5.f;
        p_io[idx * 3 + 1] = y + (ny * offset_eps) * 5.f;
        p_io[idx * 3 + 2] = z + (nz * offset_eps) * 5.f;
      }
    }
  }
}

// k_occlusion's contract (t0 = 100 eps, per-ray max_t, optional device count) with one ray per lane
template <int KIND, bool LDS>
__global__ void __launch_bounds__(kPrimBlock) k_prim_occlusion(
    const SdfDev* __restrict__ sp, const float* __restrict__ rays, int64_t P,
    const int32_t* __restrict__ count, const float* __restrict__ max_t, int max_steps, float eps,
    uint8_t* __restrict__ visible, unsigned long long* __restrict__ evals) {
  extern __shared__ float ls[];
  const SdfDev s = *sp;
  stage_table<LDS>(s, ls);
  if (count) P = min(P, (int64_t)*count);  // a compacted list (shadow rays of the hit list)
  const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = ray < P;
  if (!wave_any(valid)) return;
  const int64_t rr = valid ? ray : P - 1;
  const float ox = rays[rr * 6], oy = rays[rr * 6 + 1], oz = rays[rr * 6 + 2];
  const float dx = rays[rr * 6 + 3], dy = rays[rr * 6 + 4], dz = rays[rr * 6 + 5];
  float t = 0.f + 1e2f * eps;
  bool live = valid;
  unsigned long long nev = 0;
  for (int i = 0; i < max_steps; ++i) {
    const uint64_t lm = __ballot(live);
    if (lm == 0ull) break;
    nev += (unsigned long long)__popcll(lm);
    const float px = __fadd_rn(ox, __fmul_rn(dx, t));
    const float py = __fadd_rn(oy, __fmul_rn(dy, t));
    const float pz = __fadd_rn(oz, __fmul_rn(dz, t));
    const float d = value_at<KIND, LDS>(s, ls, px, py, pz);
    const bool now = live && (d < eps);
    if (live) t = t + d;
    live = live && !now;
  }
  if (evals && lane_id() == 0) atomicAdd(evals, nev);
  if (valid) visible[ray] = ((t >= max_t[ray]) || live) ? 1 : 0;
}

template <int KIND>
__global__ void k_pack_prims(int n, const float* __restrict__ A, const float* __restrict__ B,
                             const float* __restrict__ C, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  prim::pack<KIND>(A, B, C, i, out + (size_t)i * prim::kPrimF);
}

// ---- launch helpers ---------------------------------------------------------------------------
size_t table_lds(const nrt_sdf* s, bool lds) {
  return lds ? (size_t)s->host_dev.n_spheres * prim::kPrimF * sizeof(float) : 0;
}
bool use_lds() { return option(OPT_PRIM_MARCH) == 2; }

// KIND / LDS dispatch: F.template operator()<KIND, LDS>()
template <class F>
void prim_dispatch(const nrt_sdf* s, bool lds, F&& f) {
  if (s->host_dev.kind == prim::kBox) {
    if (lds) f.template operator()<prim::kBox, true>();
    else f.template operator()<prim::kBox, false>();
  } else {
    if (lds) f.template operator()<prim::kCapsule, true>();
    else f.template operator()<prim::kCapsule, false>();
  }
}

}  // namespace

int prim_eval(const nrt_sdf* s, const float* p, int64_t M, float* out, hipStream_t st) {
  const bool lds = use_lds();
  const size_t sh = table_lds(s, lds);
  const dim3 grid(ceil_div64(M, kPrimBlock)), block(kPrimBlock);
  prim_dispatch(s, lds, [&]<int KIND, bool LDS>() {
    k_prim_eval<KIND, LDS><<<grid, block, sh, st>>>(s->dev, p, M, out);
  });
  return check_launch("k_prim_eval");
}

int prim_intersect(const nrt_sdf* s, const float* rays, int64_t P, const MarchArgs& ma, float* t,
                   uint8_t* hit, float* p, float* n, float* raw_n, float* thr, int32_t* idx,
                   int32_t* cnt, hipStream_t st) {
  const bool lds = use_lds();
  const size_t sh = table_lds(s, lds);
  const dim3 grid(ceil_div64(P, kPrimBlock)), block(kPrimBlock);
  prim_dispatch(s, lds, [&]<int KIND, bool LDS>() {
    k_prim_intersect<KIND, LDS><<<grid, block, sh, st>>>(s->dev, rays, P, ma, t, hit, p, n, raw_n,
                                                        thr, idx, cnt);
  });
  return check_launch("k_prim_intersect");
}

int prim_normals(const nrt_sdf* s, const float* p, const int32_t* index, const int32_t* count,
                 int64_t M, float* grad, float* n_out, float* p_io, float eps, hipStream_t st) {
  const bool lds = use_lds();
  const size_t sh = table_lds(s, lds);
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(M, kPrimBlock), 4096));
  ProfScope prof("k_prim_normals", st);
  prim_dispatch(s, lds, [&]<int KIND, bool LDS>() {
    k_prim_normals<KIND, LDS><<<dim3(blocks), dim3(kPrimBlock), sh, st>>>(s->dev, p, index, count, M,
                                                                         grad, n_out, p_io, eps);
  });
  return check_launch("k_prim_normals");
}

int prim_occlusion(const nrt_sdf* s, const float* rays, int64_t P, const int32_t* count,
                   const float* max_t, int32_t max_steps, float eps, uint8_t* visible,
                   unsigned long long* evals, hipStream_t st) {
  const bool lds = use_lds();
  const size_t sh = table_lds(s, lds);
  const dim3 grid(ceil_div64(P, kPrimBlock)), block(kPrimBlock);
  prim_dispatch(s, lds, [&]<int KIND, bool LDS>() {
    k_prim_occlusion<KIND, LDS><<<grid, block, sh, st>>>(s->dev, rays, P, count, max_t, max_steps,
                                                        eps, visible, evals);
  });
  return check_launch("k_prim_occlusion");
}

// ---- training: value, gradient and parameter gradients of the smooth-min -------------------------
// The structure of nrt_sphere_smoothmin.hip: the forward is one launch; the backward is a per-point
// pass (1 / S or 0 when clamped, gamma), a (primitive, point slice) grid that sums each slice in a
// fixed order, and a reduce over the slices in order -- deterministic.
namespace {

constexpr int64_t kSliceMin = 4096;  // points per backward slice at least
constexpr int kMaxSlices = 32;
constexpr int kMaxFields = 15;

int bwd_slices(int64_t P) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxSlices, (P + kSliceMin - 1) / kSliceMin));
}
int grid_for(int64_t P) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(P, kPrimBlock), 4096));
}

// the packed table into LDS from the module's tensors
template <int KIND>
__device__ __forceinline__ void stage_params(float* ls, const float* __restrict__ A,
                                             const float* __restrict__ B,
                                             const float* __restrict__ C, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) prim::pack<KIND>(A, B, C, i, ls + i * prim::kPrimF);
  __syncthreads();
}

template <int KIND>
__global__ void __launch_bounds__(kPrimBlock) k_prim_sm_fwd(
    const float* __restrict__ p, int64_t P, const float* __restrict__ A, const float* __restrict__ B,
    const float* __restrict__ C, int n, float k, float* __restrict__ value,
    float* __restrict__ grad) {
  extern __shared__ float ls[];
  stage_params<KIND>(ls, A, B, C, n);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
    if (grad) {
      float g[3];
      const float S = prim::table_grad<KIND>((const float*)ls, n, k, x, y, z, g);
      grad[i * 3] = g[0]; grad[i * 3 + 1] = g[1]; grad[i * 3 + 2] = g[2];
      if (value) value[i] = -logf(fmaxf(S, prim::kSumMin)) / k;
    } else {
      value[i] = prim::table_value<KIND>((const float*)ls, n, k, x, y, z);
    }
  }
}

// per point: (1 / S or 0 when clamped, gamma = sum_j alpha_j beta_j)
template <int KIND>
__global__ void __launch_bounds__(kPrimBlock) k_prim_sm_pre(
    const float* __restrict__ p, int64_t P, const float* __restrict__ A, const float* __restrict__ B,
    const float* __restrict__ C, int n, float k, const float* __restrict__ dgrad,
    float2* __restrict__ pre) {
  extern __shared__ float ls[];
  stage_params<KIND>(ls, A, B, C, n);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
    float S = 0.f, wb = 0.f;
    if (dgrad) {
      const float v0 = dgrad[i * 3], v1 = dgrad[i * 3 + 1], v2 = dgrad[i * 3 + 2];
      const float* s = ls;
      for (int j = 0; j < n; ++j, s += prim::kPrimF) {
        float nn[3];
        const float w = expf(-k * prim::prim_sd_n<KIND>(s, x, y, z, nn));
        S += w;
        wb = fmaf(w, fmaf(v2, nn[2], fmaf(v1, nn[1], v0 * nn[0])), wb);
      }
    } else {
      const float* s = ls;
      for (int j = 0; j < n; ++j, s += prim::kPrimF) S += expf(-k * prim::prim_sd<KIND>(s, x, y, z));
    }
    const bool live = S >= prim::kSumMin;
    pre[i] = make_float2(live ? 1.f / S : 0.f, live ? wb / S : 0.f);
  }
}

// block (primitive j, slice): the parameter gradients summed over the slice's points in a fixed
// order, into part[(j S + slice) NF + f]
template <int KIND>
__global__ void __launch_bounds__(kPrimBlock) k_prim_sm_bwd(
    const float* __restrict__ p, int64_t P, const float* __restrict__ A, const float* __restrict__ B,
    const float* __restrict__ C, int n, float k, const float* __restrict__ dvalue,
    const float* __restrict__ dgrad, const float2* __restrict__ pre, float* __restrict__ part) {
  constexpr int NF = prim::Fields<KIND>::N;
  __shared__ float red[NF][kPrimBlock];
  __shared__ float sj[prim::kPrimF];
  const int j = blockIdx.x;
  const int S = (int)gridDim.y;
  if (threadIdx.x == 0) prim::pack<KIND>(A, B, C, j, sj);
  __syncthreads();
  float s[prim::kPrimF];
#pragma unroll
  for (int f = 0; f < prim::kPrimF; ++f) s[f] = sj[f];
  const int64_t per = (P + S - 1) / S;
  const int64_t i0 = (int64_t)blockIdx.y * per, i1 = std::min<int64_t>(P, i0 + per);
  float acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = 0.f;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    const float2 pr = pre[i];
    if (pr.x == 0.f) continue;  // clamped: v constant, g = 0
    const float x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
    const float dv = dvalue ? dvalue[i] : 0.f;
    float dg[3] = {0.f, 0.f, 0.f};
    if (dgrad) { dg[0] = dgrad[i * 3]; dg[1] = dgrad[i * 3 + 1]; dg[2] = dgrad[i * 3 + 2]; }
    prim::accumulate<KIND>((const float*)s, x, y, z, k, pr.x, pr.y, dv, dgrad != nullptr, dg, acc);
  }
  // block reduction, fixed order (deterministic)
#pragma unroll
  for (int f = 0; f < NF; ++f) red[f][threadIdx.x] = acc[f];
  __syncthreads();
  for (int w = kPrimBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int f = 0; f < NF; ++f) red[f][threadIdx.x] += red[f][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < NF) part[((int64_t)j * S + blockIdx.y) * NF + threadIdx.x] = red[threadIdx.x][0];
}

// (primitive j, field f): the slices' partial sums in slice order, into the tensors' layouts
template <int KIND>
__global__ void k_prim_sm_reduce(const float* __restrict__ part, int n, int S,
                                 float* __restrict__ dA, float* __restrict__ dB,
                                 float* __restrict__ dC) {
  constexpr int NF = prim::Fields<KIND>::N;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * NF) return;
  const int j = e / NF, f = e % NF;
  float r = 0.f;
  for (int s = 0; s < S; ++s) r += part[((int64_t)j * S + s) * NF + f];
  if (KIND == prim::kBox) {
    if (f < 9) { if (dC) dC[j * 9 + f] = r; }
    else if (f < 12) { if (dA) dA[j * 3 + (f - 9)] = r; }
    else if (dB) dB[j * 3 + (f - 12)] = r;
  } else {
    if (f < 3) { if (dA) dA[j * 3 + f] = r; }
    else if (f < 6) { if (dB) dB[j * 3 + (f - 3)] = r; }
    else if (dC) dC[j] = r;
  }
}

bool kind_ok(int kind) { return kind == prim::kBox || kind == prim::kCapsule; }

int create_prims(int kind, const char* what, int32_t n, const float* A, const float* B,
                 const float* C, float k, nrt_sdf** out) {
  if (n < 1 || !A || !B || !C || !out || !(k > 0.f)) {
    set_error(std::string(what) + ": bad argument");
    return NRT_EINVAL;
  }
  if (n > prim::kMaxPrims) {
    set_error(std::string(what) + ": more than 1024 primitives");
    return NRT_EINVAL;
  }
  std::unique_ptr<nrt_sdf> s(new nrt_sdf());
  std::memset(&s->host_dev, 0, sizeof(SdfDev));
  std::vector<float> packed((size_t)n * prim::kPrimF, 0.f);
  for (int i = 0; i < n; ++i) {
    if (kind == prim::kBox) prim::pack<prim::kBox>(A, B, C, i, &packed[(size_t)i * prim::kPrimF]);
    else prim::pack<prim::kCapsule>(A, B, C, i, &packed[(size_t)i * prim::kPrimF]);
  }
  NRT_HIP(hipMalloc(&s->spheres, packed.size() * sizeof(float)));
  NRT_HIP(hipMemcpy(s->spheres, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
  s->host_dev.kind = kind;
  s->host_dev.n_spheres = n;
  s->host_dev.k = k;
  s->host_dev.spheres = s->spheres;
  s->host_dev.mlp = nullptr;
  s->host_dev.nb = 0;
  NRT_HIP(hipMalloc(&s->dev, sizeof(SdfDev)));
  NRT_HIP(hipMemcpy(s->dev, &s->host_dev, sizeof(SdfDev), hipMemcpyHostToDevice));
  *out = s.release();
  return NRT_OK;
}

int refresh_prims(int kind, const char* what, nrt_sdf* s, const float* A, const float* B,
                  const float* C, void* stream) {
  if (!s || !A || !B || !C) { set_error(std::string(what) + ": null argument"); return NRT_EINVAL; }
  if (s->host_dev.kind != kind || !s->spheres) {
    set_error(std::string(what) + ": not an SDF of this kind");
    return NRT_EINVAL;
  }
  const int n = s->host_dev.n_spheres;
  const dim3 grid((n + 255) / 256), block(256);
  if (kind == prim::kBox) k_pack_prims<prim::kBox><<<grid, block, 0, (hipStream_t)stream>>>(n, A, B, C, s->spheres);
  else k_pack_prims<prim::kCapsule><<<grid, block, 0, (hipStream_t)stream>>>(n, A, B, C, s->spheres);
  return check_launch("k_pack_prims");
}

template <int KIND>
int sm_backward(const float* p, int64_t P, const float* A, const float* B, const float* C, int n,
                float k, const float* dvalue, const float* dgrad, float* dA, float* dB, float* dC,
                void* workspace, hipStream_t st) {
  constexpr int NF = prim::Fields<KIND>::N;
  const size_t lds = (size_t)n * prim::kPrimF * sizeof(float);
  float2* pre = (float2*)workspace;
  float* part = (float*)((char*)workspace + (((size_t)P * sizeof(float2) + 255) & ~(size_t)255));
  const int S = bwd_slices(P);
  k_prim_sm_pre<KIND><<<dim3(grid_for(P)), dim3(kPrimBlock), lds, st>>>(p, P, A, B, C, n, k, dgrad, pre);
  if (int rc = check_launch("k_prim_sm_pre")) return rc;
  k_prim_sm_bwd<KIND><<<dim3(n, S), dim3(kPrimBlock), 0, st>>>(p, P, A, B, C, n, k, dvalue, dgrad,
                                                               pre, part);
  if (int rc = check_launch("k_prim_sm_bwd")) return rc;
  k_prim_sm_reduce<KIND><<<dim3((n * NF + 255) / 256), dim3(256), 0, st>>>(part, n, S, dA, dB, dC);
  return check_launch("k_prim_sm_reduce");
}

}  // namespace
}  // namespace nrt

using namespace nrt;

extern "C" {

int nrt_sdf_create_round_boxes(int32_t n, const float* centers, const float* b, const float* tfs,
                               float k, nrt_sdf** out) {
  return create_prims(prim::kBox, "nrt_sdf_create_round_boxes", n, centers, b, tfs, k, out);
}

int nrt_sdf_create_capsules(int32_t n, const float* a, const float* b, const float* radii, float k,
                            nrt_sdf** out) {
  return create_prims(prim::kCapsule, "nrt_sdf_create_capsules", n, a, b, radii, k, out);
}

int nrt_sdf_refresh_round_boxes(nrt_sdf* s, const float* centers, const float* b, const float* tfs,
                                void* stream) {
  return refresh_prims(prim::kBox, "nrt_sdf_refresh_round_boxes", s, centers, b, tfs, stream);
}

int nrt_sdf_refresh_capsules(nrt_sdf* s, const float* a, const float* b, const float* radii,
                             void* stream) {
  return refresh_prims(prim::kCapsule, "nrt_sdf_refresh_capsules", s, a, b, radii, stream);
}

size_t nrt_prim_smoothmin_workspace_bytes(int64_t P) {
  const size_t pre = ((size_t)std::max<int64_t>(P, 1) * sizeof(float2) + 255) & ~(size_t)255;
  return pre + (size_t)prim::kMaxPrims * bwd_slices(P) * kMaxFields * sizeof(float);
}

int nrt_prim_smoothmin_forward(int32_t kind, const float* p, int64_t P, const float* A,
                               const float* B, const float* C, int32_t n, float k, float* value,
                               float* grad, void* stream) {
  if (!kind_ok(kind) || P < 0 || n < 1 || n > prim::kMaxPrims || !A || !B || !C || !(k > 0.f)) {
    set_error("nrt_prim_smoothmin_forward: bad argument (kind 3 / 4, 1 <= n <= 1024)");
    return NRT_EINVAL;
  }
  if (P == 0 || (!value && !grad)) return NRT_OK;
  if (!p) { set_error("nrt_prim_smoothmin_forward: null points"); return NRT_EINVAL; }
  const size_t lds = (size_t)n * prim::kPrimF * sizeof(float);
  const dim3 grid(grid_for(P)), block(kPrimBlock);
  hipStream_t st = (hipStream_t)stream;
  if (kind == prim::kBox) k_prim_sm_fwd<prim::kBox><<<grid, block, lds, st>>>(p, P, A, B, C, n, k, value, grad);
  else k_prim_sm_fwd<prim::kCapsule><<<grid, block, lds, st>>>(p, P, A, B, C, n, k, value, grad);
  return check_launch("k_prim_sm_fwd");
}

int nrt_prim_smoothmin_backward(int32_t kind, const float* p, int64_t P, const float* A,
                                const float* B, const float* C, int32_t n, float k,
                                const float* dvalue, const float* dgrad, float* dA, float* dB,
                                float* dC, void* workspace, void* stream) {
  if (!kind_ok(kind) || P < 0 || n < 1 || n > prim::kMaxPrims || !A || !B || !C || !(k > 0.f)) {
    set_error("nrt_prim_smoothmin_backward: bad argument (kind 3 / 4, 1 <= n <= 1024)");
    return NRT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  if (P == 0 || (!dvalue && !dgrad)) {  // no gradient flows: zeros
    const size_t c_bytes = kind == prim::kBox ? (size_t)n * 36 : (size_t)n * 4;
    if (dA) NRT_HIP(hipMemsetAsync(dA, 0, (size_t)n * 12, st));
    if (dB) NRT_HIP(hipMemsetAsync(dB, 0, (size_t)n * 12, st));
    if (dC) NRT_HIP(hipMemsetAsync(dC, 0, c_bytes, st));
    return NRT_OK;
  }
  if (!p || !workspace) { set_error("nrt_prim_smoothmin_backward: null points / workspace"); return NRT_EINVAL; }
  if (kind == prim::kBox)
    return sm_backward<prim::kBox>(p, P, A, B, C, n, k, dvalue, dgrad, dA, dB, dC, workspace, st);
  return sm_backward<prim::kCapsule>(p, P, A, B, C, n, k, dvalue, dgrad, dA, dB, dC, workspace, st);
}

}  // extern "C"
