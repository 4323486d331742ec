// gvrs_lsop_lu.h -- JAMA's LU and solve of the bordered normal equations of the optimal predictors, on one wave: the 13 x 13
// system of LSOP12 (gvrs_lsop.hip) and the 9 x 9 system of LSOP08 (gvrs_lsop8.hip).  Include inside the kernel file's anonymous
// namespace.
#pragma once

__device__ __forceinline__ double lsop_bcast(double x, int k)           // value of lane k (k wave-uniform)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), k), hi = __builtin_amdgcn_readlane(__double2hiint(x), k);
    return __hiloint2double(hi, lo);
}

// JAMA's LU (LUDecomposition.java:70-134) and solve (:253-284) of the N x N system of LsOptimalPredictor12.computeCoefficients
// :353-378 (N = 13) or LsOptimalPredictor08.computeCoefficients :211-239 (N = 9) on one wave: lane i holds row i in registers.
// S.G holds the sums of products of z0 .. z(N-1) and z(N) = 1 as the upper triangle (i <= j) without its last element.  The reference's
// inner loop  s += LU[i][k] * LUcolj[k]  runs over k in the same order here, for all rows in lockstep (row i stops at
// k = min(i, j)); the column value of row k is final exactly when step k needs it.  Every multiply and add is
// rounded separately, as in Java.  Writes S.u / S.status.
template <int N, class Shared>                         // Shared: G, u, status
__device__ __forceinline__ void lsop_lu_solve_wave(Shared &S, int lane)
{
    auto Cij = [&](int i, int j) -> double {              // c[i][j], symmetric (:345-349)
        if (i > j) { const int q = i; i = j; j = q; }
        return S.G[i * (N + 1) - (i * (i - 1)) / 2 + (j - i)];
    };
    auto Si = [&](int i) -> double { return S.G[i * (N + 1) - (i * (i - 1)) / 2 + (N - i)]; };
    const int row = lane < N ? lane : N - 1;              // lanes >= N shadow the last row (results unused)
    double r[N], x;
#pragma unroll
    for (int j = 0; j < N - 1; j++) r[j] = row < N - 1 ? Cij(row + 1, j + 1) : Si(j + 1);
    r[N - 1] = row < N - 1 ? Si(row + 1) : 0.0;
    x = row < N - 1 ? Cij(0, row + 1) : Si(0);               // right-hand side, permuted along with the rows
    bool singular = false;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double colv = r[j], s = 0.0;
#pragma unroll
        for (int k = 0; k < j; k++) {
            const double ck = lsop_bcast(__dsub_rn(colv, s), k);      // LUcolj[k] after its own update
            if (lane > k) s = __dadd_rn(s, __dmul_rn(r[k], ck));
        }
        colv = __dsub_rn(colv, s);
        r[j] = colv;
        // pivot: first row >= j with the largest |value| (strict > in scan order)
        int p = j;
        double ap = fabs(lsop_bcast(colv, j));
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            const double ai = fabs(lsop_bcast(colv, i));
            if (ai > ap) { p = i; ap = ai; }
        }
        p = __builtin_amdgcn_readfirstlane(p);
        if (p != j) {
            const int partner = lane == j ? p : lane == p ? j : lane;
#pragma unroll
            for (int c = 0; c < N; c++) r[c] = __shfl(r[c], partner, 64);
            x = __shfl(x, partner, 64);
        }
        const double djj = lsop_bcast(r[j], j);
        if (djj != 0.0) { if (lane > j) r[j] = __ddiv_rn(r[j], djj); }
        else singular = true;
    }
    if (singular) {
        if (lane == 0) S.status = GF_K_DECLINED;          // "Matrix is singular." -> computeCoefficients returns null
        return;
    }
#pragma unroll
    for (int k = 0; k < N; k++) {                         // L y = b(piv)
        const double xk = lsop_bcast(x, k);
        if (lane > k) x = __dsub_rn(x, __dmul_rn(xk, r[k]));
    }
#pragma unroll
    for (int k = N - 1; k >= 0; k--) {                       // U x = y
        if (lane == k) x = __ddiv_rn(x, r[k]);
        const double xk = lsop_bcast(x, k);
        if (lane < k) x = __dsub_rn(x, __dmul_rn(xk, r[k]));
    }
    if (lane < N - 1) S.u[lane] = (float)x;
}
