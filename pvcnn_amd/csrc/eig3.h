// eig3.h -- the eigenvector of the smallest eigenvalue of a symmetric 3 x 3 matrix, fp64, host and device (plain C++).
//
// Cyclic Jacobi, a fixed number of sweeps over the pairs (0,1), (0,2), (1,2), every index a compile-time constant: the six matrix
// entries and the nine entries of the rotation product are named scalars, so a kernel keeps them in registers (an array indexed at
// run time would live in scratch memory; tests/test_kernel_resources.py refuses that).  No branch depends on convergence: a NaN input
// ends after the same sweeps as any other.  A rotation whose off-diagonal entry is already zero is skipped, so a matrix with an exact
// zero row (points in a coordinate plane) keeps that axis exactly.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PVCNN_HD __host__ __device__ __forceinline__
#else
#define PVCNN_HD inline
#endif

namespace pvcnn {

constexpr int kEig3Sweeps = 6;   // quadratic convergence: 4 sweeps reach fp64 round-off on a 3 x 3; two more cost nothing that matters

// One Jacobi rotation in the (p, q) plane, r the third index: app, aqq, apq the pivot block, arp, arq the third row's entries, (vip, viq)
// the columns p and q of the accumulated rotations (Numerical Recipes' update: t = sgn(th) / (|th| + sqrt(th^2 + 1)), th = (aqq - app) / 2apq).
PVCNN_HD void eig3_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p,
                          double &v1q, double &v2p, double &v2q) {
  if (apq == 0.0) return;
  const double th = (aqq - app) / (2.0 * apq);
  const double t = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));   // th^2 overflows to inf: t = 0, the rotation is the identity
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;
  v0p = c * x0 - s * y0; v0q = s * x0 + c * y0;
  v1p = c * x1 - s * y1; v1q = s * x1 + c * y1;
  v2p = c * x2 - s * y2; v2q = s * x2 + c * y2;
}

// A = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]] -> its smallest eigenvalue (returned) and a unit eigenvector of it (n0, n1, n2).
PVCNN_HD double eig3_smallest(double a00, double a01, double a02, double a11, double a12, double a22, double &n0, double &n1, double &n2) {
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#ifdef __HIPCC__
#pragma unroll 1
#endif
  for (int sweep = 0; sweep < kEig3Sweeps; ++sweep) {
    eig3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), r = 2
    eig3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), r = 1
    eig3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), r = 0
  }
  double lam;
  if (a00 <= a11 && a00 <= a22) { lam = a00; n0 = v00; n1 = v10; n2 = v20; }
  else if (a11 <= a22)          { lam = a11; n0 = v01; n1 = v11; n2 = v21; }
  else                          { lam = a22; n0 = v02; n1 = v12; n2 = v22; }
  const double inv = 1.0 / sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  n0 *= inv; n1 *= inv; n2 *= inv;
  return lam;
}

}  // namespace pvcnn
