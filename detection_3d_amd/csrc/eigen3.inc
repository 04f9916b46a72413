// The eigenvector of a symmetric 3x3's smallest eigenvalue in fp64 (consumers: normals.hip, planes.hip).  Included
// inside namespace d3d's anonymous namespace.

constexpr int kSweeps = 8;                        // cyclic Jacobi on a 3x3: converged to fp64 after 5-6

// smallest eigenvalue's unit eigenvector of the symmetric c = (xx, xy, xz, yy, yz, zz): cyclic Jacobi, fixed sweeps.
// -> false when the largest eigenvalue is not positive.
__device__ bool smallest_eigenvector(const double c[6], double out[3]) {
  double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll 1
  for (int sweep = 0; sweep < kSweeps; sweep++) {
#pragma unroll
    for (int pair = 0; pair < 3; pair++) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2, r = 3 - p - q;
      const double apq = A[p][q];
      if (apq == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
      A[p][p] -= t * apq;
      A[q][q] += t * apq;
      A[p][q] = A[q][p] = 0.0;
      const double arp = A[r][p], arq = A[r][q];
      A[r][p] = A[p][r] = cs * arp - sn * arq;
      A[r][q] = A[q][r] = sn * arp + cs * arq;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double vp = V[k][p], vq = V[k][q];
        V[k][p] = cs * vp - sn * vq;
        V[k][q] = sn * vp + cs * vq;
      }
    }
  }
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  if (!(fmax(l0, fmax(l1, l2)) > 0.0)) return false;
  const int m = (l0 <= l1 && l0 <= l2) ? 0 : (l1 <= l2 ? 1 : 2);
  double v[3] = {m == 0 ? V[0][0] : m == 1 ? V[0][1] : V[0][2], m == 0 ? V[1][0] : m == 1 ? V[1][1] : V[1][2],
                 m == 0 ? V[2][0] : m == 1 ? V[2][1] : V[2][2]};
  const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (!(len > 0.0)) return false;
  for (int k = 0; k < 3; k++) out[k] = v[k] / len;
  return true;
}
