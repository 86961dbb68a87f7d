// Test-only probe, first translation unit of tests/native/libmath_probe.so: the headers that compile for host AND device —
// csrc/libm_f32.h, csrc/libm_f64.h and include/morb/camera_math.h — each function behind a device entry (probe_*) and a host entry
// (host_*) that evaluate the SAME header text, so a test can compare the gfx950 compile with the x86-64 compile bit for bit.  Under
// hipcc camera_math.h takes atan2f / cosf / sinf / tanf from libm_f32.h in both passes.  Built by morb_slam_amd/build.py:
// build_math_probe() with the library's own flags; not part of libmorb_hip.so.
#include "math_probe_common.h"

#include "libm_f32.h"
#include "libm_f64.h"
#include "morb/camera_math.h"

// ---- libm_f32.h ------------------------------------------------------------------------------------------------------------------------
PROBE_HD(atanf, float, 1, float, 1, o[0] = morbm::atanf_glibc(a[0]);)
PROBE_HD(acosf, float, 1, float, 1, o[0] = morbm::acosf_glibc(a[0]);)
PROBE_HD(tanf, float, 1, float, 1, o[0] = morbm::tanf_glibc(a[0]);)
PROBE_HD(sinf, float, 1, float, 1, o[0] = morbm::sinf_glibc(a[0]);)
PROBE_HD(cosf, float, 1, float, 1, o[0] = morbm::cosf_glibc(a[0]);)
PROBE_HD(atan2f, float, 2, float, 1, o[0] = morbm::atan2f_glibc(a[0], a[1]);)   // (y, x)

// ---- libm_f64.h ------------------------------------------------------------------------------------------------------------------------
PROBE_HD(sin64, double, 1, double, 1, o[0] = morbm64::sin_glibc(a[0]);)
PROBE_HD(cos64, double, 1, double, 1, o[0] = morbm64::cos_glibc(a[0]);)
PROBE_HD(sincos64, double, 1, double, 2, morbm64::sincos_glibc(a[0], &o[0], &o[1]);)
PROBE_HD(exp64, double, 1, double, 1, o[0] = morbm64::exp_glibc(a[0]);)

// ---- camera_math.h ---------------------------------------------------------------------------------------------------------------------
// float records: cam = fx fy cx cy k0 k1 k2 k3, then the point (x y z) or the pixel (u v)
PROBE_HD(pinhole_project, float, 11, float, 2,
         morbcam::Camera c; c.kb8 = 0; for (int k = 0; k < 8; ++k) c.p[k] = a[k];
         morbcam::project(c, a + 8, o[0], o[1]);)
PROBE_HD(pinhole_unproject, float, 10, float, 3,
         morbcam::Camera c; c.kb8 = 0; for (int k = 0; k < 8; ++k) c.p[k] = a[k];
         morbcam::unproject(c, a[8], a[9], o);)
PROBE_HD(kb8_project, float, 11, float, 2,
         morbcam::Camera c; c.kb8 = 1; for (int k = 0; k < 8; ++k) c.p[k] = a[k];
         morbcam::project(c, a + 8, o[0], o[1]);)
PROBE_HD(kb8_unproject, float, 10, float, 3,
         morbcam::Camera c; c.kb8 = 1; for (int k = 0; k < 8; ++k) c.p[k] = a[k];
         morbcam::unproject(c, a[8], a[9], o);)
// double records: the eight camera parameters (float values held in doubles), then the point
PROBE_HD(kb8_project_d, double, 11, double, 2,
         float c[8]; for (int k = 0; k < 8; ++k) c[k] = (float)a[k];
         morbcam::kb8_project_d(c, a + 8, o);)
PROBE_HD(kb8_project_jac, double, 11, double, 6,
         float c[8]; for (int k = 0; k < 8; ++k) c[k] = (float)a[k];
         morbcam::kb8_project_jac(c, a + 8, o);)
