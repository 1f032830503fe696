// nrt_nerf_train.hip -- training path of the volumetric shapes (shapes/nerf.py: PlainNeRF :46-74,
// NeRFLE :175-214): everything between and after the two MLPs, forward and backward.  Samples
// are sample-major (i = s * P + p), one lane per ray in the compositing kernels, so a wave's
// accesses to the compact [S, P] arrays are contiguous.  Bandwidth-bound; no MFMA, no atomics.
#include "nrt_launch.h"

namespace nrt {

// defined in nrt_api_nerf.hip (k_nerf_points / k_plain_first_in): the sample points, and for
// PlainNeRF the first MLP's latent rows
int launch_nerf_points(const float* rays, int64_t P, const float* ts, int S, float* pts,
                       hipStream_t st);
int launch_plain_first_in(const float* rays, int64_t P, const float* ts, int S,
                          const float* latent, int L, int64_t rays_per_latent, float* pts,
                          float* lat1, hipStream_t st);

// ------------------------------------------------------------------------------------------
// assembly: the second MLP's inputs and the compact alpha_raw[S, P] from first_out[n, O1]
// ------------------------------------------------------------------------------------------
// Every first_out element is read once, in memory order (consecutive lanes, consecutive
// addresses): column 0 goes to alpha_raw (+ noise), column 1 + k to column k of `dst` (NeRFLE:
// x2 [n, 67 + LK], k_nerf_second_in's layout; PlainNeRF: lat2 [n, I + L], k_plain_second_in's).
template <int = 0>
__global__ void k_nerf_split_first(const float* __restrict__ first_out, int O1, int64_t n,
                                   const float* __restrict__ noise, float* __restrict__ dst,
                                   int dstride, float* __restrict__ alpha_raw) {
  const int64_t ne = n * O1;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / O1;
    const int c = (int)(e - i * O1);
    const float v = first_out[e];
    if (c == 0) alpha_raw[i] = noise ? v + noise[i] : v;
    else dst[i * dstride + (c - 1)] = v;
  }
}

// NeRFLE: columns 64.. of x2 = [r_d (3) | light (LK)]   (nerf.py:199-203); light [rows, LK],
// ray p reads row p / rpl (rpl = 0: one row for every ray)
template <int = 0>
__global__ void k_nerfle_tail_in(const float* __restrict__ rays, int64_t P, int64_t n,
                                 const float* __restrict__ light, int LK, int64_t rpl,
                                 float* __restrict__ x2) {
  const int T = 3 + LK, in2 = 67 + LK;
  const int64_t ne = n * T;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / T;
    const int c = (int)(e - i * T);
    const int64_t p = i % P;
    x2[i * in2 + 64 + c] =
        c < 3 ? rays[p * 6 + 3 + c] : light[(rpl > 0 ? (p / rpl) * LK : 0) + c - 3];
  }
}

// PlainNeRF: x2 = dir_to_elev_azim(r_d), columns I.. of lat2 = the camera's latent row
// (nerf.py:52, :60-64)
template <int = 0>
__global__ void k_plain_tail_in(const float* __restrict__ rays, int64_t P, int64_t n,
                                const float* __restrict__ latent, int L, int I,
                                int64_t rays_per_latent, float* __restrict__ x2,
                                float* __restrict__ lat2) {
  const int L2 = I + L;
  const int64_t ne = n * L;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / L;
    const int c = (int)(e - i * L);
    const int64_t p = i % P;
    lat2[i * L2 + I + c] = latent[(p / rays_per_latent) * L + c];
    if (c == 0) {
      float elev, azim;
      dir_elev_azim(rays[p * 6 + 3], rays[p * 6 + 4], rays[p * 6 + 5], elev, azim);
      x2[i * 2] = elev;
      x2[i * 2 + 1] = azim;
    }
  }
}

// d_first_out[n, O1], whole rows in memory order: column 0 from d_alpha_raw, column 1 + k from
// column k of d_src (NeRFLE: the second MLP's dx; PlainNeRF: its dlatent)
template <int = 0>
__global__ void k_nerf_join_first(const float* __restrict__ d_alpha_raw,
                                  const float* __restrict__ d_src, int sstride, int O1, int64_t n,
                                  float* __restrict__ d_first_out) {
  const int64_t ne = n * O1;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / O1;
    const int c = (int)(e - i * O1);
    d_first_out[e] = c == 0 ? d_alpha_raw[i] : d_src[i * sstride + (c - 1)];
  }
}

// ------------------------------------------------------------------------------------------
// compositing (nerf.py:64-74, :203-214), one lane per ray
// ------------------------------------------------------------------------------------------
template <bool TANH>
__device__ __forceinline__ float colour_of(float x) {
  if constexpr (TANH) return tanhf(x);
  else return 1.f / (1.f + expf(-x));
}

// The statements and their order are k_nerf_composite's / k_plain_composite's (nrt_api_nerf.hip)
// on the compact alpha_raw[s * P + p]: the frame equals theirs bit for bit.
template <bool TANH>
__global__ void k_nerf_vol_forward(const float* __restrict__ alpha_raw,
                                   const float* __restrict__ rgb_raw,
                                   const float* __restrict__ ts, int64_t P, int S,
                                   float* __restrict__ out) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P;
       p += (int64_t)gridDim.x * blockDim.x) {
    float cp = 1.f;
    for (int s = 0; s < S; ++s) {
      const float sig = fmaxf(alpha_raw[(int64_t)s * P + p], 0.f);
      const float a = 1.f - expf(-(sig * ts[s]));
      cp = cp * fmaxf(1.f - a, 1e-10f);
    }
    const float cp_last = cp;
    float acc[3] = {0.f, 0.f, 0.f};
    float prev = 1.f;  // cp_{s-1}
    for (int s = 0; s < S; ++s) {
      const int64_t i = (int64_t)s * P + p;
      const float sig = fmaxf(alpha_raw[i], 0.f);
      const float a = 1.f - expf(-(sig * ts[s]));
      const float w = s == S - 1 ? a * 1.f : (s == 0 ? a * cp_last : a * prev);
      prev = prev * fmaxf(1.f - a, 1e-10f);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] += w * colour_of<TANH>(rgb_raw[i * 3 + k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[p * 3 + k] = TANH ? (acc[k] + 1.f) / 2.f : acc[k];
  }
}

// Backward of the above.  With q_s = max(1 - a_s, 1e-10), cp_j = prod_{i<=j} q_i (cp_{-1} = 1),
// G_s = <d_acc, colour_s> and the weights w_0 = a_0 cp_{S-1}, w_s = a_s cp_{s-1}, w_{S-1} =
// a_{S-1}, the direct gradients on cp are D_{s-1} = G_s a_s (1 <= s <= S-2) and D_{S-1} = G_0 a_0
// (S > 1).  dL/dq_j = cp_{j-1} R_j with R_j = D_j + q_{j+1} R_{j+1}: one reverse recursion and no
// division by q (cp underflows on opaque rays).  The forward sweep leaves cp_{s-1} in
// cpw[s * P + p] for the reverse sweep.
template <bool TANH>
__global__ void k_nerf_vol_backward(const float* __restrict__ alpha_raw,
                                    const float* __restrict__ rgb_raw,
                                    const float* __restrict__ ts, int64_t P, int S,
                                    const float* __restrict__ d_out, float* __restrict__ cpw,
                                    float* __restrict__ d_alpha_raw,
                                    float* __restrict__ d_rgb_raw) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P;
       p += (int64_t)gridDim.x * blockDim.x) {
    float dacc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) dacc[k] = TANH ? d_out[p * 3 + k] * 0.5f : d_out[p * 3 + k];
    float prev = 1.f;
    for (int s = 0; s < S; ++s) {
      const int64_t i = (int64_t)s * P + p;
      const float sig = fmaxf(alpha_raw[i], 0.f);
      const float a = 1.f - expf(-(sig * ts[s]));
      cpw[i] = prev;
      prev = prev * fmaxf(1.f - a, 1e-10f);
    }
    const float cp_last = prev;
    float g0a0 = 0.f;  // G_0 a_0: the direct gradient on cp_{S-1}
    if (S > 1) {
      const float sig = fmaxf(alpha_raw[p], 0.f);
      const float a = 1.f - expf(-(sig * ts[0]));
      float g = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) g += dacc[k] * colour_of<TANH>(rgb_raw[p * 3 + k]);
      g0a0 = g * a;
    }
    float R_next = 0.f, q_next = 0.f, ga_next = 0.f;  // R_{s+1}, q_{s+1}, G_{s+1} a_{s+1}
    for (int s = S - 1; s >= 0; --s) {
      const int64_t i = (int64_t)s * P + p;
      const float raw = alpha_raw[i];
      const float t = ts[s];
      const float e = expf(-(fmaxf(raw, 0.f) * t));
      const float a = 1.f - e;
      const float q = fmaxf(1.f - a, 1e-10f);
      const float cpm = cpw[i];  // cp_{s-1}
      const float dwda = s == S - 1 ? 1.f : (s == 0 ? cp_last : cpm);
      const float w = a * dwda;
      float G = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float c = colour_of<TANH>(rgb_raw[i * 3 + k]);
        G += dacc[k] * c;
        const float dc = TANH ? 1.f - c * c : c * (1.f - c);
        d_rgb_raw[i * 3 + k] = w * dacc[k] * dc;
      }
      // D_s: from w_{s+1} when 1 <= s + 1 <= S - 2, from w_0 when s = S - 1
      float D = s == S - 1 ? g0a0 : (s + 1 <= S - 2 ? ga_next : 0.f);
      const float R = s == S - 1 ? D : D + q_next * R_next;
      const float dq = cpm * R;
      const float da = G * dwda - (1.f - a >= 1e-10f ? dq : 0.f);
      d_alpha_raw[i] = raw > 0.f ? da * (e * t) : 0.f;
      R_next = R;
      q_next = q;
      ga_next = G * a;
    }
  }
}

// ------------------------------------------------------------------------------------------
// reductions over samples: out[r, c] = sum over the samples of latent row r of
// A[i, a_col + c] (+ B[i, b_col + c]).  Two stages, fixed summation order, no atomics.
// Row r owns rays [r * rpl, (r + 1) * rpl) at every depth; block (b, r) sums a contiguous slice
// of that row's S * rpl samples.  Threads are (sample slot, column) with the column fastest, so
// consecutive lanes read consecutive floats of one sample's row.
// ------------------------------------------------------------------------------------------
constexpr int kRedThreads = 256;

template <int = 0>
__global__ void k_nerf_reduce_partial(const float* __restrict__ A, int astride, int a_col,
                                      const float* __restrict__ B, int bstride, int b_col,
                                      int ncols, int CP, int64_t P, int S, int64_t rpl,
                                      int64_t per_block, float* __restrict__ partial) {
  __shared__ float sm[kRedThreads];
  const int c = threadIdx.x % CP, slot = threadIdx.x / CP, slots = kRedThreads / CP;
  const int64_t r = blockIdx.y;
  const int64_t m = (int64_t)S * rpl;
  const int64_t j0 = (int64_t)blockIdx.x * per_block, j1 = j0 + per_block < m ? j0 + per_block : m;
  float acc = 0.f;
  if (c < ncols)
    for (int64_t j = j0 + slot; j < j1; j += slots) {
      const int64_t s = j / rpl;
      const int64_t i = s * P + r * rpl + (j - s * rpl);
      float v = A[i * astride + a_col + c];
      if (B) v += B[i * bstride + b_col + c];
      acc += v;
    }
  sm[threadIdx.x] = acc;
  __syncthreads();
  if (slot == 0 && c < ncols) {
    float t = sm[c];
    for (int k = 1; k < slots; ++k) t += sm[k * CP + c];
    partial[(r * gridDim.x + blockIdx.x) * ncols + c] = t;
  }
}

template <int = 0>
__global__ void k_nerf_reduce_final(const float* __restrict__ partial, int nb, int ncols,
                                    int64_t total, float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / ncols;
    const int c = (int)(e - r * ncols);
    float t = 0.f;
    for (int b = 0; b < nb; ++b) t += partial[(r * nb + b) * ncols + c];
    out[e] = t;
  }
}

// ------------------------------------------------------------------------------------------
// the rays' gradient (learnable cameras): pts = r_o + ts[s] r_d (nerf.py:51, :179) and the second
// MLP's view of r_d.  One lane per ray, s ascending: a fixed order, no atomics.
//   d_rays[p, 0:3] = sum_s d_pts[i],  d_rays[p, 3:6] = sum_s ts[s] d_pts[i] + direction term
// NERFLE: r_d is columns 64..66 of x2 (nerf.py:199-203): the term is sum_s d_second[i, 64:67].
// PLAIN: x2 = dir_to_elev_azim(r_d) (utils.py:490-494) is the same for every sample of a ray, so
// the two columns of d_second are summed first and the Jacobian applied once: through asin /
// atan2 / sqrt, the clamps (no gradient where one is active, as torch gives) and F.normalize.
// ------------------------------------------------------------------------------------------
template <bool PLAIN>
__global__ void k_nerf_rays_backward(const float* __restrict__ rays, int64_t P,
                                     const float* __restrict__ ts, int S,
                                     const float* __restrict__ d_pts,
                                     const float* __restrict__ d_second, int sstride,
                                     float* __restrict__ d_rays) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P;
       p += (int64_t)gridDim.x * blockDim.x) {
    float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      const int64_t i = (int64_t)s * P + p;
      const float t = ts[s];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float g = d_pts[i * 3 + k];
        go[k] += g;
        gd[k] += t * g;
      }
      if constexpr (PLAIN) {
        gs[0] += d_second[i * sstride];
        gs[1] += d_second[i * sstride + 1];
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) gs[k] += d_second[i * sstride + 64 + k];
      }
    }
    if constexpr (PLAIN) {
      // dir_elev_azim's statements (nrt_kernels.h) again, then their gradient
      const float vx = rays[p * 6 + 3], vy = rays[p * 6 + 4], vz = rays[p * 6 + 5];
      const float len = sqrtf(vx * vx + vy * vy + vz * vz);
      const float nrm = fmaxf(len, 1e-12f);
      const float nx = vx / nrm, ny = vy / nrm, nz = vz / nrm;
      const float lo = -1.f + 1e-7f, hi = 1.f - 1e-7f;
      const float x = fminf(fmaxf(nx, lo), hi), z = fminf(fmaxf(nz, lo), hi);
      const float w = (1.f - x * x) - z * z;
      const float q = sqrtf(fmaxf(w, 1e-10f));
      const float den = x * x + q * q;
      // elev = asin(z); azim = atan2(x, q): d/dx = q / den, d/dq = -x / den
      const float gq = w >= 1e-10f ? (-x / den) * gs[1] / (2.f * q) : 0.f;  // dL/dw
      float gx = (q / den) * gs[1] + gq * (-2.f * x);
      float gz = gs[0] / sqrtf(1.f - z * z) + gq * (-2.f * z);
      if (nx < lo || nx > hi) gx = 0.f;
      if (nz < lo || nz > hi) gz = 0.f;
      // back through n = v / max(|v|, eps): (g - n (n . g)) / |v|, g = (gx, 0, gz)
      if (len >= 1e-12f) {
        const float ng = nx * gx + nz * gz;
        gs[0] = (gx - nx * ng) / len;
        gs[1] = (0.f - ny * ng) / len;
        gs[2] = (gz - nz * ng) / len;
      } else {
        gs[0] = gx / nrm; gs[1] = 0.f; gs[2] = gz / nrm;
      }
    }
    float* o = d_rays + p * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[k] = go[k];
      o[3 + k] = gd[k] + gs[k];
    }
  }
}

static size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }
static int grid_for(int64_t elems) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((elems + 255) / 256, 8192));
}
// blocks per latent row of the first reduction stage: slices of at least kRedMinSamples samples
constexpr int64_t kRedMinSamples = 256;
constexpr int64_t kRedMaxBlocks = 256;
static int64_t reduce_blocks(int64_t samples_per_row) {
  return std::max<int64_t>(1, std::min(kRedMaxBlocks, (samples_per_row + kRedMinSamples - 1) /
                                                          kRedMinSamples));
}

}  // namespace nrt

using namespace nrt;

extern "C" {

size_t nrt_nerf_volume_workspace_bytes(int64_t P, int32_t S, int32_t dim) {
  const size_t p = (size_t)std::max<int64_t>(P, 1);
  const size_t n = p * (size_t)std::max(S, 1);
  // cp_{s-1} [S, P] of the composite backward, then the reduction's partials: at most
  // rows * reduce_blocks(S rpl) <= rows + n / kRedMinSamples rows of `dim` floats
  return a256(n * 4) + a256((p + n / (size_t)kRedMinSamples + 1) * (size_t)std::max(dim, 1) * 4);
}

int nrt_nerf_points(int32_t model, const float* rays, int64_t P, const float* ts, int32_t S,
                    const float* latent, int32_t L, int64_t rays_per_latent, float* pts,
                    float* lat1, void* stream) {
  if (P < 0 || S < 1 || (model != NRT_NERF_NERFLE && model != NRT_NERF_PLAIN)) {
    set_error("nrt_nerf_points: bad argument");
    return NRT_EINVAL;
  }
  if (P == 0) return NRT_OK;
  if (!rays || !ts || !pts) { set_error("nrt_nerf_points: null argument"); return NRT_EINVAL; }
  if (model == NRT_NERF_NERFLE) return launch_nerf_points(rays, P, ts, S, pts, (hipStream_t)stream);
  if (!latent || !lat1 || L < 1 || rays_per_latent < 1) {
    set_error("nrt_nerf_points: PlainNeRF needs latent [rows, L], lat1 and rays_per_latent >= 1");
    return NRT_EINVAL;
  }
  return launch_plain_first_in(rays, P, ts, S, latent, L, rays_per_latent, pts, lat1,
                               (hipStream_t)stream);
}

int nrt_nerf_assemble(int32_t model, const float* first_out, const float* rays, int64_t P,
                      int32_t S, const float* extra, int32_t extra_dim, int32_t I,
                      int64_t rays_per_latent, const float* noise, float* x2, float* lat2,
                      float* alpha_raw, void* stream) {
  if (P < 0 || S < 1 || extra_dim < 1 || (model != NRT_NERF_NERFLE && model != NRT_NERF_PLAIN)) {
    set_error("nrt_nerf_assemble: bad argument");
    return NRT_EINVAL;
  }
  if (P == 0) return NRT_OK;
  if (!first_out || !rays || !extra || !x2 || !alpha_raw) {
    set_error("nrt_nerf_assemble: null argument");
    return NRT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = P * (int64_t)S;
  ProfScope prof("k_nerf_assemble", st);
  if (model == NRT_NERF_NERFLE) {
    const int in2 = 67 + extra_dim;
    if (rays_per_latent > 0 && rays_per_latent < P && P % rays_per_latent != 0) {
      set_error("nrt_nerf_assemble: P must be a multiple of rays_per_latent (rays per light row)");
      return NRT_EINVAL;
    }
    k_nerf_split_first<><<<dim3(grid_for(n * 65)), dim3(256), 0, st>>>(first_out, 65, n, nullptr,
                                                                         x2, in2, alpha_raw);
    if (int rc = check_launch("k_nerf_split_first")) return rc;
    k_nerfle_tail_in<><<<dim3(grid_for(n * (3 + extra_dim))), dim3(256), 0, st>>>(
        rays, P, n, extra, extra_dim, rays_per_latent > 0 && rays_per_latent < P ? rays_per_latent : 0,
        x2);
    return check_launch("k_nerfle_tail_in");
  }
  if (!lat2 || I < 0 || rays_per_latent < 1) {
    set_error("nrt_nerf_assemble: PlainNeRF needs lat2, I >= 0 and rays_per_latent >= 1");
    return NRT_EINVAL;
  }
  k_nerf_split_first<><<<dim3(grid_for(n * (1 + I))), dim3(256), 0, st>>>(
      first_out, 1 + I, n, noise, lat2, I + extra_dim, alpha_raw);
  if (int rc = check_launch("k_nerf_split_first")) return rc;
  k_plain_tail_in<><<<dim3(grid_for(n * extra_dim)), dim3(256), 0, st>>>(
      rays, P, n, extra, extra_dim, I, rays_per_latent, x2, lat2);
  return check_launch("k_plain_tail_in");
}

int nrt_nerf_assemble_backward(int32_t model, const float* d_alpha_raw, const float* d_second,
                               int64_t P, int32_t S, int32_t extra_dim, int32_t I,
                               float* d_first_out, void* stream) {
  if (P < 0 || S < 1 || extra_dim < 1 || I < 0 ||
      (model != NRT_NERF_NERFLE && model != NRT_NERF_PLAIN)) {
    set_error("nrt_nerf_assemble_backward: bad argument");
    return NRT_EINVAL;
  }
  if (P == 0) return NRT_OK;
  if (!d_alpha_raw || !d_second || !d_first_out) {
    set_error("nrt_nerf_assemble_backward: null argument");
    return NRT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = P * (int64_t)S;
  const int O1 = model == NRT_NERF_NERFLE ? 65 : 1 + I;
  const int sstride = model == NRT_NERF_NERFLE ? 67 + extra_dim : I + extra_dim;
  ProfScope prof("k_nerf_assemble_bwd", st);
  k_nerf_join_first<><<<dim3(grid_for(n * O1)), dim3(256), 0, st>>>(d_alpha_raw, d_second, sstride,
                                                                      O1, n, d_first_out);
  return check_launch("k_nerf_join_first");
}

int nrt_nerf_composite_forward(int32_t model, const float* alpha_raw, const float* rgb_raw,
                               const float* ts, int64_t P, int32_t S, float* out, void* stream) {
  if (P < 0 || S < 1 || (model != NRT_NERF_NERFLE && model != NRT_NERF_PLAIN)) {
    set_error("nrt_nerf_composite_forward: bad argument");
    return NRT_EINVAL;
  }
  if (P == 0) return NRT_OK;
  if (!alpha_raw || !rgb_raw || !ts || !out) {
    set_error("nrt_nerf_composite_forward: null argument");
    return NRT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div64(P, 64), 65536));
  ProfScope prof("k_nerf_vol_forward", st);
  if (model == NRT_NERF_PLAIN)
    k_nerf_vol_forward<true><<<grid, dim3(64), 0, st>>>(alpha_raw, rgb_raw, ts, P, S, out);
  else
    k_nerf_vol_forward<false><<<grid, dim3(64), 0, st>>>(alpha_raw, rgb_raw, ts, P, S, out);
  return check_launch("k_nerf_vol_forward");
}

int nrt_nerf_composite_backward(int32_t model, const float* alpha_raw, const float* rgb_raw,
                                const float* ts, int64_t P, int32_t S, const float* d_out,
                                float* d_alpha_raw, float* d_rgb_raw, void* workspace,
                                void* stream) {
  if (P < 0 || S < 1 || (model != NRT_NERF_NERFLE && model != NRT_NERF_PLAIN)) {
    set_error("nrt_nerf_composite_backward: bad argument");
    return NRT_EINVAL;
  }
  if (P == 0) return NRT_OK;
  if (!alpha_raw || !rgb_raw || !ts || !d_out || !d_alpha_raw || !d_rgb_raw || !workspace) {
    set_error("nrt_nerf_composite_backward: null argument");
    return NRT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  float* cpw = (float*)workspace;
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div64(P, 64), 65536));
  ProfScope prof("k_nerf_vol_backward", st);
  if (model == NRT_NERF_PLAIN)
    k_nerf_vol_backward<true><<<grid, dim3(64), 0, st>>>(alpha_raw, rgb_raw, ts, P, S, d_out, cpw,
                                                         d_alpha_raw, d_rgb_raw);
  else
    k_nerf_vol_backward<false><<<grid, dim3(64), 0, st>>>(alpha_raw, rgb_raw, ts, P, S, d_out, cpw,
                                                          d_alpha_raw, d_rgb_raw);
  return check_launch("k_nerf_vol_backward");
}

int nrt_nerf_rays_backward(int32_t model, const float* rays, int64_t P, const float* ts, int32_t S,
                           const float* d_pts, const float* d_second, int32_t second_stride,
                           float* d_rays, void* stream) {
  if (P < 0 || S < 1 || (model != NRT_NERF_NERFLE && model != NRT_NERF_PLAIN) ||
      second_stride < (model == NRT_NERF_NERFLE ? 67 : 2)) {
    set_error("nrt_nerf_rays_backward: bad argument");
    return NRT_EINVAL;
  }
  if (P == 0) return NRT_OK;
  if (!rays || !ts || !d_pts || !d_second || !d_rays) {
    set_error("nrt_nerf_rays_backward: null argument");
    return NRT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div64(P, 64), 65536));
  ProfScope prof("k_nerf_rays_backward", st);
  if (model == NRT_NERF_PLAIN)
    k_nerf_rays_backward<true><<<grid, dim3(64), 0, st>>>(rays, P, ts, S, d_pts, d_second,
                                                          second_stride, d_rays);
  else
    k_nerf_rays_backward<false><<<grid, dim3(64), 0, st>>>(rays, P, ts, S, d_pts, d_second,
                                                           second_stride, d_rays);
  return check_launch("k_nerf_rays_backward");
}

int nrt_nerf_reduce(int32_t model, const float* d_first, const float* d_second, int64_t P,
                    int32_t S, int32_t dim, int32_t I, int64_t rays_per_latent, float* out,
                    void* workspace, void* stream) {
  if (P < 0 || S < 1 || dim < 1 || I < 0 ||
      (model != NRT_NERF_NERFLE && model != NRT_NERF_PLAIN)) {
    set_error("nrt_nerf_reduce: bad argument");
    return NRT_EINVAL;
  }
  if (dim > kRedThreads) {
    set_error("nrt_nerf_reduce: at most 256 columns");
    return NRT_EUNSUPPORTED;
  }
  if (P == 0) return NRT_OK;
  if (!d_second || !out || !workspace || (model == NRT_NERF_PLAIN && !d_first)) {
    set_error("nrt_nerf_reduce: null argument");
    return NRT_EINVAL;
  }
  // NERFLE: rays per light row; <= 0 or >= P is the one row every ray shares
  const int64_t rpl = model == NRT_NERF_PLAIN || (rays_per_latent > 0 && rays_per_latent < P)
                          ? rays_per_latent : P;
  if (rpl < 1 || P % rpl != 0) {
    set_error("nrt_nerf_reduce: P must be a multiple of rays_per_latent");
    return NRT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = P * (int64_t)S, rows = P / rpl;
  if (rows > 65535) { set_error("nrt_nerf_reduce: more than 65535 latent rows"); return NRT_EUNSUPPORTED; }
  float* partial = (float*)((char*)workspace + a256((size_t)n * 4));
  const int64_t m = (int64_t)S * rpl;
  const int64_t nb = reduce_blocks(m);
  const int64_t per_block = (m + nb - 1) / nb;
  int CP = 1;
  while (CP < dim) CP <<= 1;
  ProfScope prof("k_nerf_reduce", st);
  if (model == NRT_NERF_NERFLE)
    k_nerf_reduce_partial<><<<dim3((unsigned)nb, (unsigned)rows), dim3(kRedThreads), 0, st>>>(
        d_second, 67 + dim, 67, nullptr, 0, 0, dim, CP, P, S, rpl, per_block, partial);
  else
    k_nerf_reduce_partial<><<<dim3((unsigned)nb, (unsigned)rows), dim3(kRedThreads), 0, st>>>(
        d_first, dim, 0, d_second, I + dim, I, dim, CP, P, S, rpl, per_block, partial);
  if (int rc = check_launch("k_nerf_reduce_partial")) return rc;
  k_nerf_reduce_final<><<<dim3(grid_for(rows * dim)), dim3(256), 0, st>>>(partial, (int)nb, dim,
                                                                            rows * dim, out);
  return check_launch("k_nerf_reduce_final");
}

}  // extern "C"
