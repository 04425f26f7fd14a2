// camera model batch calls of the C-ABI (include/ptzba.h ptz_*; camera_kernels.hip)
#include <vector>

#include "../../include/ptzba.h"
#include "ptzba_kernels.h"
#include "host_util.h"

using namespace ptzba;

struct Tmp {
  std::vector<DBuf*> bufs;
  ~Tmp() {
    for (auto* b : bufs) delete b;
  }
  double* in(const double* h, size_t n) {
    auto* b = new DBuf();
    bufs.push_back(b);
    if (b->alloc(n * 8)) return nullptr;
    if (hipMemcpy(b->p, h, n * 8, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return b->as<double>();
  }
  double* out(size_t n) {
    auto* b = new DBuf();
    bufs.push_back(b);
    if (b->alloc(n * 8)) return nullptr;
    return b->as<double>();
  }
};

#define NEED(p)                                   \
  do {                                            \
    if (!(p)) return fail("device allocation/copy failed"); \
  } while (0)

int ptz_ray_to_image(int device, int64_t n, double u, double v, const double* f, const double* cp, const double* ct,
                     const double* th, const double* ph, double* x_out, double* y_out) {
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(device));
  Tmp t;
  double *df = t.in(f, n), *dcp = t.in(cp, n), *dct = t.in(ct, n), *dth = t.in(th, n), *dph = t.in(ph, n);
  double *dx = t.out(n), *dy = t.out(n);
  NEED(df && dcp && dct && dth && dph && dx && dy);
  launch_ray_to_image(n, u, v, df, dcp, dct, dth, dph, dx, dy, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(x_out, dx, n * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(y_out, dy, n * 8, hipMemcpyDeviceToHost));
  return 0;
}

int ptz_image_to_ray(int device, int64_t n, double u, double v, const double* f, const double* cp, const double* ct,
                     const double* x, const double* y, double* th_out, double* ph_out) {
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(device));
  Tmp t;
  double *df = t.in(f, n), *dcp = t.in(cp, n), *dct = t.in(ct, n), *dx = t.in(x, n), *dy = t.in(y, n);
  double *dth = t.out(n), *dph = t.out(n);
  NEED(df && dcp && dct && dx && dy && dth && dph);
  launch_image_to_ray(n, u, v, df, dcp, dct, dx, dy, dth, dph, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(th_out, dth, n * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ph_out, dph, n * 8, hipMemcpyDeviceToHost));
  return 0;
}

int ptz_project_rays(int device, int64_t n, double u, double v, double f, double pan, double tilt, const double* d6,
                     const double* rays, double* xy_out) {
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(device));
  Tmp t;
  double *dr = t.in(rays, 2 * n), *dxy = t.out(2 * n);
  NEED(dr && dxy);
  launch_project_rays(n, u, v, f, pan, tilt, d6, dr, dxy, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(xy_out, dxy, 2 * n * 8, hipMemcpyDeviceToHost));
  return 0;
}

int ptz_back_project_rays(int device, int64_t n, double u, double v, double f, double pan, double tilt,
                          const double* d6, const double* xy, double* rays_out) {
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(device));
  Tmp t;
  double *dxy = t.in(xy, 2 * n), *dr = t.out(2 * n);
  NEED(dxy && dr);
  launch_back_project(n, u, v, f, pan, tilt, d6, dxy, dr, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(rays_out, dr, 2 * n * 8, hipMemcpyDeviceToHost));
  return 0;
}

int ptz_back_project_rays_exact(int device, int64_t n, double u, double v, double f, double pan, double tilt,
                                const double* d6, const double* xy, double* rays_out, uint8_t* valid_out) {
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  if (!xy || !rays_out) return fail("null argument");
  if (d6)
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(d6[k])) return fail("displacement: non-finite value at index %d", k);
  HIPCHK(hipSetDevice(device));
  Tmp t;
  double *dxy = t.in(xy, 2 * n), *dr = t.out(2 * n);
  DBuf dvalid;
  NEED(dxy && dr && dvalid.alloc((size_t)n) == 0);
  launch_back_project_exact(n, u, v, f, pan, tilt, d6, dxy, dr, dvalid.as<uint8_t>(), nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(rays_out, dr, 2 * n * 8, hipMemcpyDeviceToHost));
  if (valid_out) HIPCHK(hipMemcpy(valid_out, dvalid.p, (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

int ptz_h_jacobian(int device, int64_t n, double u, double v, double f, double pan, double tilt, const double* d6,
                   const double* rays, double* H_out) {
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(device));
  Tmp t;
  const size_t nh = (size_t)(2 * n) * (size_t)(3 + 2 * n);
  double *dr = t.in(rays, 2 * n), *dH = t.out(nh);
  NEED(dr && dH);
  HIPCHK(hipMemset(dH, 0, nh * 8));
  launch_h_jacobian(n, u, v, f, pan, tilt, d6, dr, dH, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(H_out, dH, nh * 8, hipMemcpyDeviceToHost));
  return 0;
}
