// FP32 / fp32-split forward-mode SDF normals on the ring32 / ring3 engines (k_normal32 /
// k_normal3 = k_normal_r, nrt_kernels.h): the normal pass of nrt_sdf_intersect after a ring32 /
// ring3 march, in place of the per-wave reverse-mode k_sdf_grad.
#include "nrt_launch.h"

namespace nrt {

int ring_normals32(const nrt_sdf* s, const int32_t* idx, const int32_t* cnt, int64_t M, float* grad,
                   float* n, float* p_io, float eps, bool split, hipStream_t st) {
  const MlpDev& md = s->mlp->host_dev;
  const size_t bias = ring_bias_bytes(s), sph = ring32_sphere_bytes(s);
  // 4 rays per wave; blocks stride over the device-side hit count
  auto launch = [&](auto kern, size_t lds, int WV, const char* name) -> int {
    if (int rc = set_lds(kern, lds)) return rc;
    const int blocks = resident_grid(kern, 64 * WV, lds, ceil_div64(M, 4 * WV));
    ProfScope prof(name, st);
    kern<<<dim3(blocks), dim3(64 * WV), lds, st>>>(s->host_dev, md, idx, cnt, M, grad, n, p_io, eps);
    return check_launch(name);
  };
  if (split)
    return ring3_dispatch(s, [&]<int KH, int KQ, int ACT>() -> int {
      using E = ring3::Engine<KH, KQ, kRing3Waves>;
      return launch(k_normal_r<RingPol3<KH, KQ, kRing3Waves, ACT>>, E::lds_bytes(md.freqs, bias, sph),
                    kRing3Waves, "k_normal3");
    });
  return ring32_dispatch(s, [&]<int KH, int KE, int ACT>() -> int {
    using E = ring32::Engine<KH, KE, kRing32Waves>;
    return launch(k_normal_r<RingPol32<KH, KE, kRing32Waves, ACT>>, E::lds_bytes(md.freqs, bias, sph),
                  kRing32Waves, "k_normal32");
  });
}

}  // namespace nrt
