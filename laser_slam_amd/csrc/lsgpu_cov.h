// lsgpu_cov.h -- host side of PointToPlaneWithCovErrorMinimizer (include/lsgpu_icp.h): the six step
// parameters the covariance kernel takes, and the 6x6 work on its 44 sums.  Host only, double throughout; the library calls
// these after the loop and lsgpu_point_to_plane_cov_solve hands the second one out, so the two agree bit for bit.
#pragma once
#include <cmath>
#include "../../include/lsgpu_icp.h"

namespace lsgpu {
namespace cov {

constexpr int kSums = 44;   // 21 upper-tri of H, 21 of M, the pair count, sum (n . (p - q))^2

// {alpha, beta, gamma, tx, ty, tz} of the step dT (4x4 float, column major): the angles in double, rounded to float
inline void step_params(const float dT[16], float wt[6]) {
  auto at = [&](int r, int c) { return (double)dT[c * 4 + r]; };
  const double beta = -std::asin(at(2, 0));
  const double alpha = std::atan2(at(2, 1), at(2, 2));
  const double cb = std::cos(beta);
  const double gamma = std::atan2(at(1, 0) / cb, at(0, 0) / cb);
  wt[0] = (float)alpha; wt[1] = (float)beta; wt[2] = (float)gamma;
  wt[3] = dT[12]; wt[4] = dT[13]; wt[5] = dT[14];
}

// cov = sigma^2 H^-1 M H^-1 (row major, the upper triangle computed and mirrored).  false: singular -- a non-finite sum or
// result, or a Cholesky pivot of H no greater than 1e-6 of its own diagonal entry; cov is then left as it was.
inline bool solve(const double sums[kSums], double sigma, double cov[36]) {
  for (int i = 0; i < 42; ++i)
    if (!(sums[i] - sums[i] == 0.0)) return false;
  double H[6][6], M[6][6];
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c, ++k) { H[a][c] = H[c][a] = sums[k]; M[a][c] = M[c][a] = sums[21 + k]; }
  double L[6][6] = {};
  for (int j = 0; j < 6; ++j) {
    double s = H[j][j];
    for (int q = 0; q < j; ++q) s -= L[j][q] * L[j][q];
    if (!(s > 1e-6 * H[j][j])) return false;
    L[j][j] = std::sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double t = H[i][j];
      for (int q = 0; q < j; ++q) t -= L[i][q] * L[j][q];
      L[i][j] = t / L[j][j];
    }
  }
  double Li[6][6] = {};   // L^-1 (lower triangular), column by column
  for (int c = 0; c < 6; ++c)
    for (int i = c; i < 6; ++i) {
      double t = i == c ? 1.0 : 0.0;
      for (int q = c; q < i; ++q) t -= L[i][q] * Li[q][c];
      Li[i][c] = t / L[i][i];
    }
  double Hi[6][6];        // H^-1 = L^-T L^-1
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c) {
      double t = 0.0;
      for (int q = c; q < 6; ++q) t += Li[q][a] * Li[q][c];
      Hi[a][c] = Hi[c][a] = t;
    }
  double X[6][6];         // H^-1 M
  for (int a = 0; a < 6; ++a)
    for (int c = 0; c < 6; ++c) {
      double t = 0.0;
      for (int q = 0; q < 6; ++q) t += Hi[a][q] * M[q][c];
      X[a][c] = t;
    }
  const double s2 = sigma * sigma;
  double out[36];
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c) {
      double t = 0.0;
      for (int q = 0; q < 6; ++q) t += X[a][q] * Hi[q][c];
      t = s2 * t;
      if (!(t - t == 0.0)) return false;
      out[a * 6 + c] = out[c * 6 + a] = t;
    }
  for (int i = 0; i < 36; ++i) cov[i] = out[i];
  return true;
}

}  // namespace cov
}  // namespace lsgpu
