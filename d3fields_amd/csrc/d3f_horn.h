// d3f_horn.h -- Horn's closed-form rotation from a 3 x 3 cross-covariance, in float64 (shared by pose_refit_kernel of consensus_kernels.hip
// and motion_fit_kernel of motion_kernels.hip; restated line for line in tests/consensus_cases.py and tests/motion_cases.py).
//
// S_ab = sum (p - pm)_a (c - cm)_b.  The symmetric 4 x 4 matrix N of S, its eigenvectors by kHornSweeps cyclic Jacobi sweeps over (i < j) in
// row order (a zero off-diagonal entry is skipped), the column of the largest diagonal entry (the first among equals) as the quaternion
// (q0, q1, q2, q3), R = the quaternion's matrix divided by |q|^2.  Only IEEE + - * / sqrt in the stated order; nothing fused.
//
// A and V are the caller's 4 x 4 work matrices, entry (i, j) at [(4 * i + j) * STRIDE]: they are indexed dynamically, so they belong in LDS
// (in registers that would go to scratch).  One lane works on one pair of matrices; STRIDE > 1 interleaves the matrices of several lanes.
#pragma once
#include <hip/hip_runtime.h>

namespace d3f {

constexpr int kHornSweeps = 12;

template <int STRIDE>
__device__ __forceinline__ void horn_rotation(const double (&S)[3][3], double *__restrict__ A, double *__restrict__ V, double (&R)[3][3])
{
#define D3F_HORN_A(i, j) A[(4 * (i) + (j)) * STRIDE]
#define D3F_HORN_V(i, j) V[(4 * (i) + (j)) * STRIDE]
    D3F_HORN_A(0, 0) = (S[0][0] + S[1][1]) + S[2][2];
    D3F_HORN_A(1, 1) = (S[0][0] - S[1][1]) - S[2][2];
    D3F_HORN_A(2, 2) = (S[1][1] - S[0][0]) - S[2][2];
    D3F_HORN_A(3, 3) = (S[2][2] - S[0][0]) - S[1][1];
    D3F_HORN_A(0, 1) = D3F_HORN_A(1, 0) = S[1][2] - S[2][1];
    D3F_HORN_A(0, 2) = D3F_HORN_A(2, 0) = S[2][0] - S[0][2];
    D3F_HORN_A(0, 3) = D3F_HORN_A(3, 0) = S[0][1] - S[1][0];
    D3F_HORN_A(1, 2) = D3F_HORN_A(2, 1) = S[0][1] + S[1][0];
    D3F_HORN_A(1, 3) = D3F_HORN_A(3, 1) = S[2][0] + S[0][2];
    D3F_HORN_A(2, 3) = D3F_HORN_A(3, 2) = S[1][2] + S[2][1];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) D3F_HORN_V(i, j) = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kHornSweeps; ++sweep) {
#pragma unroll 1
        for (int i = 0; i < 3; ++i) {
#pragma unroll 1
            for (int j = i + 1; j < 4; ++j) {
                const double apq = D3F_HORN_A(i, j);
                if (apq == 0.0) continue;
                const double theta = (D3F_HORN_A(j, j) - D3F_HORN_A(i, i)) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                D3F_HORN_A(i, i) -= t * apq;
                D3F_HORN_A(j, j) += t * apq;
                D3F_HORN_A(i, j) = D3F_HORN_A(j, i) = 0.0;
                for (int m = 0; m < 4; ++m) {
                    if (m != i && m != j) {
                        const double ami = D3F_HORN_A(m, i), amj = D3F_HORN_A(m, j);
                        D3F_HORN_A(m, i) = D3F_HORN_A(i, m) = c * ami - s * amj;
                        D3F_HORN_A(m, j) = D3F_HORN_A(j, m) = s * ami + c * amj;
                    }
                    const double vmi = D3F_HORN_V(m, i), vmj = D3F_HORN_V(m, j);
                    D3F_HORN_V(m, i) = c * vmi - s * vmj;
                    D3F_HORN_V(m, j) = s * vmi + c * vmj;
                }
            }
        }
    }
    int top = 0;
    for (int i = 1; i < 4; ++i)
        if (D3F_HORN_A(i, i) > D3F_HORN_A(top, top)) top = i;
    const double q0 = D3F_HORN_V(0, top), q1 = D3F_HORN_V(1, top), q2 = D3F_HORN_V(2, top), q3 = D3F_HORN_V(3, top);
    const double a0 = q0 * q0, a1 = q1 * q1, a2 = q2 * q2, a3 = q3 * q3, n2 = ((a0 + a1) + a2) + a3;
    R[0][0] = (((a0 + a1) - a2) - a3) / n2;
    R[0][1] = (2.0 * (q1 * q2 - q0 * q3)) / n2;
    R[0][2] = (2.0 * (q1 * q3 + q0 * q2)) / n2;
    R[1][0] = (2.0 * (q1 * q2 + q0 * q3)) / n2;
    R[1][1] = (((a0 - a1) + a2) - a3) / n2;
    R[1][2] = (2.0 * (q2 * q3 - q0 * q1)) / n2;
    R[2][0] = (2.0 * (q1 * q3 - q0 * q2)) / n2;
    R[2][1] = (2.0 * (q2 * q3 + q0 * q1)) / n2;
    R[2][2] = (((a0 - a1) - a2) + a3) / n2;
#undef D3F_HORN_A
#undef D3F_HORN_V
}

}  // namespace d3f
