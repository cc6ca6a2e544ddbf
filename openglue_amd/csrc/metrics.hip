// The reference's validation metrics (utils/metrics.py, called from models/matching_module.py:107-131):
//
//  * og_epipolar_precision -- AccuracyUsingEpipolarDist: per pair, the kornia symmetric epipolar distance (squared form) of
//    every match under E = [T]x R, in fp64; precision = correct / matched, matching score = correct / detected.
//      precision_kernel   one workgroup per pair, a fixed-order block reduction of two integer counts
//
//  * og_essential_5pt -- the five-point minimal solver (Nister / Stewenius), fp64 throughout, one thread per problem:
//      solve_poly_kernel  the 4-d null space of the 5 x 9 epipolar constraints (Gauss-Jordan, then Gram-Schmidt), the ten cubic
//                         constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 as a 10 x 20 matrix, eliminated in LDS
//                         (Gauss-Jordan with partial pivoting); the three hidden-variable rows <e>-z<f>, <g>-z<h>, <i>-z<j>
//                         are written out with the null-space basis
//      solve_roots_kernel det of the 3 x 3 polynomial matrix (degree 10 in z), Sturm sequence, bisection on the Sturm count
//                         for every real root, two Newton steps, back-substitution for x, y, Gauss-Newton on the ten constraints;
//                         E = x X + y Y + z Z + W, unit norm, kept when every constraint holds to 1e-9
//    Between the two kernels the intermediate state of a problem lives in its own 90 output slots (E [count][10][9]), so the
//    entry needs no workspace: the second kernel reads all of it before it writes any solution.
//
//  * og_relative_pose -- CameraPoseAUC's pose: RANSAC over the same solver, then kornia's cheirality choice.
//      prep_kernel        one workgroup per pair: the valid matches compacted in index order, calibrated points, the threshold
//      solve_poly_kernel  one thread per (pair, hypothesis): 5 distinct matches drawn by a counter-based hash
//      solve_roots_kernel
//      score_kernel       one model (hypothesis, solution) per lane, the pair's points staged through LDS, squared Sampson
//                         error <= thr^2 in fp32 on the unit-norm E; the best model per pair is a packed 64-bit atomicMax of
//                         (inliers + 1, ~model index): most inliers, lowest index on ties, identical from run to run
//      finish_kernel      one workgroup per pair: inlier mask, SVD of E (Jacobi on E^T E, fp64), the four (R, t), depth
//                         checks spread over lanes, errors against the ground truth
//    Every launch count is fixed: 5 kernels whatever the batch.
#include "og_common.h"
#include "og_ransac.h"      // finite, pmul, peval, mix64, draw_distinct, to_f4, publish_best, jacobi3; og_block.h: block_sum

namespace {

constexpr int kMaxSol = 10;
constexpr int kSlots = 90;          // doubles per problem in the E buffer: 10 solutions x 9
constexpr int kPolyLds = 64;        // problems (threads) per solve_poly workgroup: 64 x 200 doubles of LDS

// ------------------------------------------------------------------------------------------------ five-point solver
// Monomials of degree <= 3 in (x, y, z) in the order of the elimination (Stewenius):
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__host__ __device__ constexpr int mono(int a, int b, int c) {
    return a == 3 ? 0 : b == 3 ? 1 : (a == 2 && b == 1) ? 2 : (a == 1 && b == 2) ? 3 : (a == 2 && c == 1) ? 4 : a == 2 ? 5
         : (b == 2 && c == 1) ? 6 : b == 2 ? 7 : (a == 1 && b == 1 && c == 1) ? 8 : (a == 1 && b == 1) ? 9
         : (a == 1 && c == 2) ? 10 : (a == 1 && c == 1) ? 11 : a == 1 ? 12 : (b == 1 && c == 2) ? 13 : (b == 1 && c == 1) ? 14
         : b == 1 ? 15 : c == 3 ? 16 : c == 2 ? 17 : c == 1 ? 18 : 19;
}
// a linear form has the coefficients of (x, y, z, 1); a quadratic one those of the products v_i v_j, i <= j
__host__ __device__ constexpr int ex(int v) { return v == 0; }
__host__ __device__ constexpr int ey(int v) { return v == 1; }
__host__ __device__ constexpr int ez(int v) { return v == 2; }
__host__ __device__ constexpr int qidx(int i, int j) { return i * 4 - i * (i - 1) / 2 + (j - i); }

struct Lin { double c[4]; };
struct Quad { double c[10]; };

__host__ __device__ inline Quad qmul(const Lin& a, const Lin& b) {
    Quad q;
#pragma unroll
    for (int i = 0; i < 10; ++i) q.c[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) q.c[qidx(i < j ? i : j, i < j ? j : i)] += a.c[i] * b.c[j];
    return q;
}
__host__ __device__ inline Quad qadd(const Quad& a, const Quad& b, double sb) {
    Quad q;
#pragma unroll
    for (int i = 0; i < 10; ++i) q.c[i] = a.c[i] + sb * b.c[i];
    return q;
}
// out (20 cubic coefficients) += s * q * l
__host__ __device__ inline void cmul_acc(const Quad& q, const Lin& l, double s, double (&out)[20]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                out[mono(ex(i) + ex(j) + ex(k), ey(i) + ey(j) + ey(k), ez(i) + ez(j) + ez(k))] += s * q.c[qidx(i, j)] * l.c[k];
}

// The elimination below pivots in columns 0..4 and fixes the coefficient of W at 1, which singles out entries of E: with the
// translation along camera 1's optical axis the third row of E = [T]x R is zero, the solution lies at infinity of that chart and
// is lost; with R = I as well, columns 1 and 3 of the constraints coincide and a pivot is rounding noise.  So the solver works in
// coordinates reflected by a fixed Householder matrix H = I - 2 v v^T / |v|^2 with nine generic entries: the constraint rows
// before the elimination, the null-space basis after Gram-Schmidt (H is a symmetric involution).  No entry of E is special then.
__host__ __device__ inline void reflect9(double (&r)[9]) {
    constexpr double v[9] = {0.31, -0.27, 0.35, 0.29, -0.33, 0.26, -0.34, 0.28, 0.32};
    double vv = 0.0, d = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) { vv += v[c] * v[c]; d += r[c] * v[c]; }
    const double f = 2.0 * d / vv;
#pragma unroll
    for (int c = 0; c < 9; ++c) r[c] -= f * v[c];
}

// Stage 1 of the solver for one problem.  x0, x1: 5 calibrated points each ([5][2]).  A: the 10 x 20 elimination matrix,
// element (r, c) at A[(r * 20 + c) * S].  inter: 76 doubles at stride IS (basis X Y Z W [4][9], then the coefficients of
// the three rows of B(z) = [[kx ky k1] [lx ly l1] [mx my m1]] (x / y: 4 ascending in z, 1: 5), then 1.0 if the problem is sound).
__host__ __device__ inline void essential_poly(const double* x0, const double* x1, double* A, int S, double* inter, int IS) {
    double Q[5][9];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const double u0 = x0[2 * r], v0 = x0[2 * r + 1], u1 = x1[2 * r], v1 = x1[2 * r + 1];
        // x1^T E x0 = sum_ij x1_i E_ij x0_j, E row-major
        Q[r][0] = u1 * u0; Q[r][1] = u1 * v0; Q[r][2] = u1;
        Q[r][3] = v1 * u0; Q[r][4] = v1 * v0; Q[r][5] = v1;
        Q[r][6] = u0;      Q[r][7] = v0;      Q[r][8] = 1.0;
        reflect9(Q[r]);
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int r = k + 1; r < 5; ++r) {
            const bool sw = fabs(Q[r][k]) > fabs(Q[k][k]);
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double a = Q[k][c], b = Q[r][c];
                Q[k][c] = sw ? b : a;
                Q[r][c] = sw ? a : b;
            }
        }
        const double piv = Q[k][k];
        ok = ok && fabs(piv) > 1e-300;
        const double inv = 1.0 / piv;
#pragma unroll
        for (int c = 0; c < 9; ++c) Q[k][c] *= inv;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            if (r == k) continue;
            const double f = Q[r][k];
#pragma unroll
            for (int c = 0; c < 9; ++c) Q[r][c] -= f * Q[k][c];
        }
    }
    // null space: free columns 5..8; then modified Gram-Schmidt for conditioning
    double Nb[4][9];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
        for (int p = 0; p < 5; ++p) Nb[f][p] = -Q[p][5 + f];
#pragma unroll
        for (int g = 0; g < 4; ++g) Nb[f][5 + g] = f == g ? 1.0 : 0.0;
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
        for (int g = 0; g < f; ++g) {
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < 9; ++c) d += Nb[f][c] * Nb[g][c];
#pragma unroll
            for (int c = 0; c < 9; ++c) Nb[f][c] -= d * Nb[g][c];
        }
        double n2 = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) n2 += Nb[f][c] * Nb[f][c];
        const double inv = 1.0 / sqrt(n2);
#pragma unroll
        for (int c = 0; c < 9; ++c) Nb[f][c] *= inv;
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) reflect9(Nb[f]);      // back to the entries of E; H is orthogonal, the basis stays orthonormal
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int c = 0; c < 9; ++c) inter[(f * 9 + c) * IS] = Nb[f][c];

    // E = x X + y Y + z Z + W, entrywise linear forms
    Lin E[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = Lin{{Nb[0][e], Nb[1][e], Nb[2][e], Nb[3][e]}};
    Quad EEt[6];                                  // (00 01 02 11 12 22)
#pragma unroll
    for (int i = 0, u = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j, ++u) {
            Quad q = qmul(E[i * 3], E[j * 3]);
            q = qadd(q, qmul(E[i * 3 + 1], E[j * 3 + 1]), 1.0);
            EEt[u] = qadd(q, qmul(E[i * 3 + 2], E[j * 3 + 2]), 1.0);
        }
    auto sym = [&](int i, int j) -> const Quad& {
        const int a = i < j ? i : j, b = i < j ? j : i;
        return EEt[a * 3 - a * (a - 1) / 2 + (b - a)];
    };
    const Quad tr = qadd(qadd(EEt[0], EEt[3], 1.0), EEt[5], 1.0);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double row[20];
#pragma unroll
            for (int c = 0; c < 20; ++c) row[c] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) cmul_acc(sym(i, k), E[k * 3 + j], 2.0, row);
            cmul_acc(tr, E[i * 3 + j], -1.0, row);
#pragma unroll
            for (int c = 0; c < 20; ++c) A[((i * 3 + j) * 20 + c) * S] = row[c];
        }
    {
        double row[20];
#pragma unroll
        for (int c = 0; c < 20; ++c) row[c] = 0.0;
        cmul_acc(qadd(qmul(E[4], E[8]), qmul(E[5], E[7]), -1.0), E[0], 1.0, row);
        cmul_acc(qadd(qmul(E[3], E[8]), qmul(E[5], E[6]), -1.0), E[1], -1.0, row);
        cmul_acc(qadd(qmul(E[3], E[7]), qmul(E[4], E[6]), -1.0), E[2], 1.0, row);
#pragma unroll
        for (int c = 0; c < 20; ++c) A[(9 * 20 + c) * S] = row[c];
    }
    // Gauss-Jordan on the 10 x 20 matrix, partial pivoting (rolled loops: the matrix is addressed through A)
    for (int k = 0; k < 10; ++k) {
        int p = k;
        double best = fabs(A[(k * 20 + k) * S]);
        for (int r = k + 1; r < 10; ++r) {
            const double v = fabs(A[(r * 20 + k) * S]);
            if (v > best) { best = v; p = r; }
        }
        ok = ok && best > 1e-300;
        if (p != k)
            for (int c = k; c < 20; ++c) {
                const double t = A[(k * 20 + c) * S];
                A[(k * 20 + c) * S] = A[(p * 20 + c) * S];
                A[(p * 20 + c) * S] = t;
            }
        const double inv = 1.0 / A[(k * 20 + k) * S];
        for (int c = k; c < 20; ++c) A[(k * 20 + c) * S] *= inv;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = A[(r * 20 + k) * S];
            for (int c = k; c < 20; ++c) A[(r * 20 + c) * S] -= f * A[(k * 20 + c) * S];
        }
    }
    // <e> - z<f>, <g> - z<h>, <i> - z<j> (rows 4..9 = x^2z x^2 y^2z y^2 xyz xy): polynomials in z multiplying x, y and 1
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int a = 4 + 2 * t, b = a + 1;
        auto g = [&](int r, int c) { return A[(r * 20 + c) * S]; };
        double* o = inter + (36 + 13 * t) * IS;
        o[0 * IS] = g(a, 12); o[1 * IS] = g(a, 11) - g(b, 12); o[2 * IS] = g(a, 10) - g(b, 11); o[3 * IS] = -g(b, 10);
        o[4 * IS] = g(a, 15); o[5 * IS] = g(a, 14) - g(b, 15); o[6 * IS] = g(a, 13) - g(b, 14); o[7 * IS] = -g(b, 13);
        o[8 * IS] = g(a, 19); o[9 * IS] = g(a, 18) - g(b, 19); o[10 * IS] = g(a, 17) - g(b, 18); o[11 * IS] = g(a, 16) - g(b, 17);
        o[12 * IS] = -g(b, 16);
    }
    inter[75 * IS] = ok ? 1.0 : 0.0;
}

__host__ __device__ constexpr int soff(int k) { return 11 * k - k * (k - 1) / 2; }   // offset of Sturm polynomial k (degree 10 - k)

__host__ __device__ inline int sign_changes(const double (&s)[66], double t) {
    int n = 0, last = 0;
#pragma unroll
    for (int k = 0; k <= 10; ++k) {
        double v = s[soff(k) + 10 - k];
#pragma unroll
        for (int i = 9 - k; i >= 0; --i) v = v * t + s[soff(k) + i];
        const int sg = (v > 0.0) - (v < 0.0);
        n += (sg != 0 && last != 0 && sg != last);
        last = sg != 0 ? sg : last;
    }
    return n;
}

// the ten constraints at E = x X + y Y + z Z + W: r[0..8] = 2 E E^T E - tr(E E^T) E, r[9] = det E
__host__ __device__ inline void constraints(const double (&E)[9], double (&r)[10]) {
    double EEt[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) EEt[i * 3 + j] = E[i * 3] * E[j * 3] + E[i * 3 + 1] * E[j * 3 + 1] + E[i * 3 + 2] * E[j * 3 + 2];
    const double tr = EEt[0] + EEt[4] + EEt[8];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            r[i * 3 + j] = 2.0 * (EEt[i * 3] * E[j] + EEt[i * 3 + 1] * E[3 + j] + EEt[i * 3 + 2] * E[6 + j]) - tr * E[i * 3 + j];
    r[9] = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
}

// Up to kPolishSteps Gauss-Newton steps on (x, y, z) against the ten constraints (forward-difference Jacobian), each kept only if it
// lowers the residual: the roots of the eliminated polynomial carry the rounding of the elimination, this takes it back out.  A
// root ends the loop at its first step that does not improve, which for a well-conditioned elimination is the second or third.
// Where the leading 10 x 10 block is badly conditioned in this chart (about 1 problem in 600) the root of the eliminated
// polynomial can be 0.02 off in z; Gauss-Newton then contracts by only ~5x a step before it turns quadratic and needs ten steps to
// reach the 1e-9 keep rule (three left it at 6e-5 and the true solution was dropped).
constexpr int kPolishSteps = 12;
__host__ __device__ inline void polish(const double (&basis)[36], double& x, double& y, double& z) {
    auto build = [&](double a, double b, double c, double (&E)[9]) {
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = a * basis[k] + b * basis[9 + k] + c * basis[18 + k] + basis[27 + k];
    };
    auto norm2 = [](const double (&r)[10]) { double t = 0.0;
#pragma unroll
        for (int k = 0; k < 10; ++k) t += r[k] * r[k];
        return t; };
#pragma unroll 1
    for (int it = 0; it < kPolishSteps; ++it) {
        double E[9], r0[10], J[3][10];
        build(x, y, z, E);
        constraints(E, r0);
        const double f0 = norm2(r0);
        const double p[3] = {x, y, z};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double h = 1e-7 * fmax(1.0, fabs(p[d]));
            double Eh[9], rh[10];
            build(d == 0 ? x + h : x, d == 1 ? y + h : y, d == 2 ? z + h : z, Eh);
            constraints(Eh, rh);
#pragma unroll
            for (int k = 0; k < 10; ++k) J[d][k] = (rh[k] - r0[k]) / h;
        }
        double A[3][3], g[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            g[a] = 0.0;
#pragma unroll
            for (int k = 0; k < 10; ++k) g[a] += J[a][k] * r0[k];
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                A[a][b] = 0.0;
#pragma unroll
                for (int k = 0; k < 10; ++k) A[a][b] += J[a][k] * J[b][k];
            }
        }
        // solve A d = -g by Cramer's rule
        const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                           A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
        if (!(fabs(det) > 0.0)) return;
        double dv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double M[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) M[a][b] = b == c ? -g[a] : A[a][b];
            dv[c] = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                     M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])) / det;
        }
        double En[9], rn[10];
        build(x + dv[0], y + dv[1], z + dv[2], En);
        constraints(En, rn);
        if (!(norm2(rn) < f0)) return;
        x += dv[0]; y += dv[1]; z += dv[2];
    }
}

// Stage 2: the intermediate state of one problem (read in full first) -> up to 10 unit-norm essential matrices.  Returns their count.
__host__ __device__ inline int essential_roots(const double* inter, int IS, double* Eout) {
    double basis[36], bc[39];
#pragma unroll
    for (int i = 0; i < 36; ++i) basis[i] = inter[i * IS];
#pragma unroll
    for (int i = 0; i < 39; ++i) bc[i] = inter[(36 + i) * IS];
    if (!(inter[75 * IS] == 1.0)) return 0;
    typedef double P3[4];
    typedef double P4[5];
    const P3& kx = *(const P3*)&bc[0];  const P3& ky = *(const P3*)&bc[4];  const P4& k1 = *(const P4*)&bc[8];
    const P3& lx = *(const P3*)&bc[13]; const P3& ly = *(const P3*)&bc[17]; const P4& l1 = *(const P4*)&bc[21];
    const P3& mx = *(const P3*)&bc[26]; const P3& my = *(const P3*)&bc[30]; const P4& m1 = *(const P4*)&bc[34];
    double t0[8], t1[8], c0[11], u0[7], u1[7], c2[11];
    double s[66];
    pmul(ly, m1, t0); pmul(my, l1, t1);                    // kx (ly m1 - l1 my)
#pragma unroll
    for (int i = 0; i < 8; ++i) t0[i] -= t1[i];
    pmul(kx, t0, c0);
#pragma unroll
    for (int i = 0; i < 11; ++i) s[i] = c0[i];
    pmul(lx, m1, t0); pmul(mx, l1, t1);                    // - ky (lx m1 - l1 mx)
#pragma unroll
    for (int i = 0; i < 8; ++i) t0[i] -= t1[i];
    pmul(ky, t0, c0);
#pragma unroll
    for (int i = 0; i < 11; ++i) s[i] -= c0[i];
    pmul(lx, my, u0); pmul(ly, mx, u1);                    // + k1 (lx my - ly mx)
#pragma unroll
    for (int i = 0; i < 7; ++i) u0[i] -= u1[i];
    pmul(k1, u0, c2);
#pragma unroll
    for (int i = 0; i < 11; ++i) s[i] += c2[i];
    const double lead = s[10];
    if (!(fabs(lead) > 0.0) || !finite(lead)) return 0;
    double bound = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) s[i] /= lead;             // monic p0
#pragma unroll
    for (int i = 0; i < 10; ++i) bound = fmax(bound, fabs(s[i]));
    if (!finite(bound)) return 0;
    bound += 1.0;                                          // Cauchy: every root lies in (-bound, bound)
    // Sturm sequence p1 = p0', p_{k+1} = -rem(p_{k-1}, p_k), each scaled by a positive factor
#pragma unroll
    for (int i = 0; i < 10; ++i) s[soff(1) + i] = (i + 1) * s[i + 1] * 0.1;
#pragma unroll
    for (int k = 1; k < 10; ++k) {
        const int n = 10 - k;
        const double* a = &s[soff(k - 1)];
        const double* b = &s[soff(k)];
        const double q1 = a[n + 1] / b[n];
        const double q0 = (a[n] - q1 * b[n - 1]) / b[n];
        double mx_ = 0.0;
#pragma unroll
        for (int i = 0; i < n; ++i) {
            const double r = -(a[i] - (i > 0 ? q1 * b[i - 1] : 0.0) - q0 * b[i]);
            s[soff(k + 1) + i] = r;
            mx_ = fmax(mx_, fabs(r));
        }
        const double sc = mx_ > 0.0 ? 1.0 / mx_ : 1.0;
#pragma unroll
        for (int i = 0; i < n; ++i) s[soff(k + 1) + i] *= sc;
    }
    int vneg = 0, vpos = 0, lneg = 0, lpos = 0;
#pragma unroll
    for (int k = 0; k <= 10; ++k) {
        const double l = s[soff(k) + 10 - k];
        const int sp = (l > 0.0) - (l < 0.0);
        const int sn = ((10 - k) & 1) ? -sp : sp;
        vpos += (sp != 0 && lpos != 0 && sp != lpos); lpos = sp != 0 ? sp : lpos;
        vneg += (sn != 0 && lneg != 0 && sn != lneg); lneg = sn != 0 ? sn : lneg;
    }
    int nroots = vneg - vpos;
    nroots = nroots < 0 ? 0 : (nroots > kMaxSol ? kMaxSol : nroots);
    double lo = -bound;
    int nsol = 0;
    for (int j = 0; j < nroots; ++j) {
        double a = lo, b = bound;
        for (int it = 0; it < 160; ++it) {
            const double mid = 0.5 * (a + b);
            if (!(mid > a && mid < b)) break;
            if (vneg - sign_changes(s, mid) > j) b = mid; else a = mid;
        }
        lo = a;
        double z = 0.5 * (a + b);
#pragma unroll
        for (int it = 0; it < 2; ++it) {                   // Newton on the monic p0
            double p = 1.0, d = 0.0;
#pragma unroll
            for (int i = 9; i >= 0; --i) { d = d * z + p; p = p * z + s[i]; }
            const double zn = z - p / d;
            if (finite(zn) && fabs(zn - z) <= 1e-6 * fmax(1.0, fabs(z))) z = zn;
        }
        // x, y from B(z) [x y 1]^T = 0: the cross product of the two rows that give the largest one
        double r[3][3];
        r[0][0] = peval<4>(kx, z); r[0][1] = peval<4>(ky, z); r[0][2] = peval<5>(k1, z);
        r[1][0] = peval<4>(lx, z); r[1][1] = peval<4>(ly, z); r[1][2] = peval<5>(l1, z);
        r[2][0] = peval<4>(mx, z); r[2][1] = peval<4>(my, z); r[2][2] = peval<5>(m1, z);
        double v[3] = {0.0, 0.0, 0.0}, bn = -1.0;
#pragma unroll
        for (int pa = 0; pa < 3; ++pa) {
            const int i0 = pa == 2 ? 1 : 0, i1 = pa == 0 ? 1 : 2;
            const double cx = r[i0][1] * r[i1][2] - r[i0][2] * r[i1][1];
            const double cy = r[i0][2] * r[i1][0] - r[i0][0] * r[i1][2];
            const double cz = r[i0][0] * r[i1][1] - r[i0][1] * r[i1][0];
            const double nn = cx * cx + cy * cy + cz * cz;
            if (nn > bn) { bn = nn; v[0] = cx; v[1] = cy; v[2] = cz; }
        }
        double x = v[0] / v[2], y = v[1] / v[2];
        polish(basis, x, y, z);
        double e[9], n2 = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) { e[c] = x * basis[c] + y * basis[9 + c] + z * basis[18 + c] + basis[27 + c]; n2 += e[c] * e[c]; }
        const double inv = 1.0 / sqrt(n2);
        if (!finite(inv) || !finite(x) || !finite(y)) continue;
#pragma unroll
        for (int c = 0; c < 9; ++c) e[c] *= inv;
        // a root the polish could not bring onto the constraints (a near-double root, a spurious one) is not an essential matrix
        double res[10], worst = 0.0;
        constraints(e, res);
#pragma unroll
        for (int k = 0; k < 10; ++k) worst = fmax(worst, fabs(res[k]));
        if (!(worst <= 1e-9)) continue;
#pragma unroll
        for (int c = 0; c < 9; ++c) Eout[nsol * 9 + c] = e[c];
        ++nsol;
    }
    return nsol;
}

// ------------------------------------------------------------------------------------------------ sampling
struct PoseWs {
    double4* pts;          // [B][m] calibrated (u0, v0, u1, v1) of every keypoint with a valid match
    int* idx;              // [B][m] the valid keypoints in index order
    int* count;            // [B]
    float* thr2;           // [B] squared threshold, calibrated units
    unsigned long long* best;   // [B] packed (inliers + 1, ~model)
    double* E;             // [B * H][90]
    int* nsol;             // [B * H]
};

static size_t pose_bytes(int B, int m, int H) {
    const int64_t bm = (int64_t)B * m, bh = (int64_t)B * H;
    return og_round_up(32 * bm, 256) + og_round_up(4 * bm, 256) + og_round_up(4 * (int64_t)B, 256) + og_round_up(4 * (int64_t)B, 256) +
           og_round_up(8 * (int64_t)B, 256) + og_round_up(8 * kSlots * bh, 256) + og_round_up(4 * bh, 256);
}

static PoseWs pose_layout(void* ws, int B, int m, int H) {
    PoseWs w{};
    char* p = (char*)ws;
    const int64_t bm = (int64_t)B * m, bh = (int64_t)B * H;
    auto take = [&](int64_t bytes) { char* r = p; p += og_round_up(bytes, 256); return r; };
    w.pts = (double4*)take(32 * bm);
    w.idx = (int*)take(4 * bm);
    w.count = (int*)take(4 * (int64_t)B);
    w.thr2 = (float*)take(4 * (int64_t)B);
    w.best = (unsigned long long*)take(8 * (int64_t)B);
    w.E = (double*)take(8 * kSlots * bh);
    w.nsol = (int*)take(4 * bh);
    return w;
}

struct SolveSrc {
    // direct problems (og_essential_5pt)
    const double* x0; const double* x1;      // [count][5][2]
    // RANSAC draws (og_relative_pose): problem = b * H + h
    const double4* pts; const int* idx; const int* cnt;
    int m, H;
    uint64_t seed;
    int64_t pair_offset;
};

__global__ void __launch_bounds__(kPolyLds) solve_poly_kernel(SolveSrc src, int count, double* E) {
    __shared__ double lds[200 * kPolyLds];
    const int p = blockIdx.x * kPolyLds + threadIdx.x;
    if (p >= count) return;
    double x0[10], x1[10];
    double* inter = E + (int64_t)p * kSlots;
    if (src.x0) {
#pragma unroll
        for (int i = 0; i < 10; ++i) { x0[i] = src.x0[(int64_t)p * 10 + i]; x1[i] = src.x1[(int64_t)p * 10 + i]; }
    } else {
        const int b = p / src.H, h = p - b * src.H;
        const int n = src.cnt[b];
        if (n < 5) { inter[75] = 0.0; return; }
        int pick[5];
        draw_distinct<5>(src.seed, (uint64_t)(src.pair_offset + b), h, n, pick);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int r = pick[j];
            const double4 q = src.pts[(int64_t)b * src.m + src.idx[(int64_t)b * src.m + r]];
            x0[2 * j] = q.x; x0[2 * j + 1] = q.y; x1[2 * j] = q.z; x1[2 * j + 1] = q.w;
        }
    }
    essential_poly(x0, x1, lds + threadIdx.x, kPolyLds, inter, 1);
}

__global__ void __launch_bounds__(256) solve_roots_kernel(int count, double* E, int* nsol) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= count) return;
    double* e = E + (int64_t)p * kSlots;
    nsol[p] = essential_roots(e, 1, e);
}

// ------------------------------------------------------------------------------------------------ epipolar precision
struct Geo {
    const float* k0; const float* k1; const int64_t* matches0; const int32_t* nk0;
    const float* K0; const float* K1; const float* R; const float* T;
    int B, m, n;
};

// calibrated (x - c) / f in fp64, utils/misc.py:5-7
__device__ inline double4 calibrate(const Geo& g, int b, int i, int j) {
    const float* K0 = g.K0 + b * 9; const float* K1 = g.K1 + b * 9;
    const float2 a = ((const float2*)g.k0)[(int64_t)b * g.m + i];
    const float2 c = ((const float2*)g.k1)[(int64_t)b * g.n + j];
    return make_double4(((double)a.x - K0[2]) / K0[0], ((double)a.y - K0[5]) / K0[4],
                        ((double)c.x - K1[2]) / K1[0], ((double)c.y - K1[5]) / K1[4]);
}

__global__ void __launch_bounds__(256) precision_kernel(Geo g, double threshold, float* precision, float* matching_score, int* num_correct) {
#pragma clang fp contract(off)
    __shared__ int red[4];
    const int b = blockIdx.x;
    const float* R = g.R + b * 9; const float* T = g.T + b * 3;
    // E = [T]x R (kornia essential_from_Rt with camera 0 at the identity)
    const double t0 = T[0], t1 = T[1], t2 = T[2];
    const double tx[9] = {0.0, -t2, t1, t2, 0.0, -t0, -t1, t0, 0.0};
    double E[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) E[r * 3 + c] = tx[r * 3] * (double)R[c] + tx[r * 3 + 1] * (double)R[3 + c] + tx[r * 3 + 2] * (double)R[6 + c];
    int matched = 0, correct = 0;
    for (int i = threadIdx.x; i < g.m; i += blockDim.x) {
        int j;
        if (!valid_match(g, b, i, j)) continue;
        const double4 q = calibrate(g, b, i, j);
        const double l0 = E[0] * q.x + E[1] * q.y + E[2], l1 = E[3] * q.x + E[4] * q.y + E[5], l2 = E[6] * q.x + E[7] * q.y + E[8];
        const double m0 = E[0] * q.z + E[3] * q.w + E[6], m1 = E[1] * q.z + E[4] * q.w + E[7];
        const double num = q.z * l0 + q.w * l1 + l2;
        const double d = num * num * (1.0 / (l0 * l0 + l1 * l1) + 1.0 / (m0 * m0 + m1 * m1));
        ++matched;
        correct += d < threshold;
    }
    matched = block_sum(matched, red);
    correct = block_sum(correct, red);
    if (threadIdx.x == 0) {
        const int det = g.nk0 ? min(g.nk0[b], g.m) : g.m;
        precision[b] = matched > 0 ? (float)correct / (float)matched : 0.0f;
        matching_score[b] = matched > 0 ? (float)correct / (float)det : 0.0f;
        num_correct[b] = correct;
    }
}

// ------------------------------------------------------------------------------------------------ relative pose
__global__ void __launch_bounds__(256) prep_kernel(Geo g, float ransac_threshold, PoseWs w) {
    __shared__ int wsum[4];
    const int b = blockIdx.x;
    const int base = compact_valid_matches(g, b, w.idx + (int64_t)b * g.m, wsum,
                                           [&](int i, int j) { w.pts[(int64_t)b * g.m + i] = calibrate(g, b, i, j); });
    if (threadIdx.x == 0) {
        const float* K0 = g.K0 + b * 9; const float* K1 = g.K1 + b * 9;
        // utils/metrics.py:90 in fp32: 2 thr / mean(K0[0,0] + K1[0,0], K0[1,1] + K1[1,1])
        const float mean = ((K0[0] + K1[0]) + (K0[4] + K1[4])) / 2.0f;
        const float thr = (2.0f * ransac_threshold) / mean;
        w.count[b] = base;
        w.thr2[b] = thr * thr;
        w.best[b] = 0ull;
    }
}

// squared Sampson error <= thr^2 (OpenCV's essential-matrix error), fp32, explicit FMAs: the score and finish kernels agree bitwise
__device__ __forceinline__ bool sampson_inlier(const float (&e)[9], float4 q, float t2) {
    const float a0 = __fmaf_rn(e[0], q.x, __fmaf_rn(e[1], q.y, e[2]));
    const float a1 = __fmaf_rn(e[3], q.x, __fmaf_rn(e[4], q.y, e[5]));
    const float a2 = __fmaf_rn(e[6], q.x, __fmaf_rn(e[7], q.y, e[8]));
    const float b0 = __fmaf_rn(e[0], q.z, __fmaf_rn(e[3], q.w, e[6]));
    const float b1 = __fmaf_rn(e[1], q.z, __fmaf_rn(e[4], q.w, e[7]));
    const float num = __fmaf_rn(q.z, a0, __fmaf_rn(q.w, a1, a2));
    const float den = __fmaf_rn(a0, a0, __fmaf_rn(a1, a1, __fmaf_rn(b0, b0, __fmul_rn(b1, b1))));
    return __fdiv_rn(__fmul_rn(num, num), den) <= t2;
}

constexpr int kScoreChunk = 1024;

__global__ void __launch_bounds__(256) score_kernel(PoseWs w, int m, int H, int groups) {
    __shared__ float4 pts[kScoreChunk];
    const int b = blockIdx.x / groups;                       // `groups` workgroups per pair, pair-major along x
    const int model = (blockIdx.x - b * groups) * 256 + threadIdx.x;        // h * 10 + s
    const int h = model / kMaxSol, s = model - h * kMaxSol;
    const int64_t prob = (int64_t)b * H + h;
    const bool live = h < H && s < w.nsol[prob];
    float e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) e[c] = live ? (float)w.E[prob * kSlots + s * 9 + c] : 0.0f;
    const int n = w.count[b];
    const float t2 = w.thr2[b];
    int inl = 0;
    for (int k0 = 0; k0 < n; k0 += kScoreChunk) {
        const int len = min(kScoreChunk, n - k0);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += 256) pts[k] = to_f4(w.pts[(int64_t)b * m + w.idx[(int64_t)b * m + k0 + k]]);
        __syncthreads();
        if (live)
            for (int k = 0; k < len; ++k) inl += sampson_inlier(e, pts[k], t2);
    }
    const unsigned long long key = live ? ((unsigned long long)(inl + 1) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)model) : 0ull;
    publish_best(key, &w.best[b]);
}

__device__ inline double det3(const double (&M)[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

__global__ void __launch_bounds__(256) finish_kernel(Geo g, PoseWs w, int H, float* error, float* R_pred, float* t_pred,
                                                     uint8_t* inliers, int* num_inliers) {
    __shared__ double cand[4][12];       // R (9) and t (3) of the four candidates, kornia's order
    __shared__ int red[4];
    const int b = blockIdx.x;
    const unsigned long long key = w.best[b];
    const bool have = key != 0ull && w.count[b] >= 5;
    const int model = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    const int h = model / kMaxSol, s = model - h * kMaxSol;
    const double* Ed = w.E + ((int64_t)b * H + (have ? h : 0)) * kSlots + (have ? s : 0) * 9;
    float e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) e[c] = have ? (float)Ed[c] : 0.0f;
    const float t2 = w.thr2[b];
    if (threadIdx.x == 0 && have) {
        double Em[3][3], A[3][3], V[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Em[r][c] = Ed[r * 3 + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) A[r][c] = Em[0][r] * Em[0][c] + Em[1][r] * Em[1][c] + Em[2][r] * Em[2][c];
        jacobi3(A, V);
        // singular values descending: order the eigenvalues
        int o0 = 0, o1 = 1, o2 = 2;
        auto swp = [](int& a, int& b2) { const int t = a; a = b2; b2 = t; };
        if (A[o1][o1] > A[o0][o0]) swp(o0, o1);
        if (A[o2][o2] > A[o0][o0]) swp(o0, o2);
        if (A[o2][o2] > A[o1][o1]) swp(o1, o2);
        double U[3][3], Vs[3][3];
        const int ord[3] = {o0, o1, o2};
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int r = 0; r < 3; ++r) Vs[r][k] = V[r][ord[k]];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            double u[3], n2 = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) { u[r] = Em[r][0] * Vs[0][k] + Em[r][1] * Vs[1][k] + Em[r][2] * Vs[2][k]; n2 += u[r] * u[r]; }
            const double inv = 1.0 / sqrt(n2);
#pragma unroll
            for (int r = 0; r < 3; ++r) U[r][k] = u[r] * inv;
        }
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
        // kornia decompose_essential_matrix: flip the last column of U / the last row of V^T when the determinant is negative
        if (det3(U) < 0.0)
#pragma unroll
            for (int r = 0; r < 3; ++r) U[r][2] = -U[r][2];
        if (det3(Vs) < 0.0)
#pragma unroll
            for (int r = 0; r < 3; ++r) Vs[r][2] = -Vs[r][2];
        // W = [[0 -1 0] [1 0 0] [0 0 1]]: R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2]
        double R1[3][3], R2[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // (U W)[r] = (U[r][1], -U[r][0], U[r][2]); (U W^T)[r] = (-U[r][1], U[r][0], U[r][2])
                R1[r][c] = U[r][1] * Vs[c][0] - U[r][0] * Vs[c][1] + U[r][2] * Vs[c][2];
                R2[r][c] = -U[r][1] * Vs[c][0] + U[r][0] * Vs[c][1] + U[r][2] * Vs[c][2];
            }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) cand[k][r * 3 + c] = k < 2 ? R1[r][c] : R2[r][c];
#pragma unroll
            for (int r = 0; r < 3; ++r) cand[k][9 + r] = (k & 1) ? -U[r][2] : U[r][2];
        }
    }
    __syncthreads();
    int inl = 0, pos[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < g.m; i += blockDim.x) {
        int j;
        bool f = false;
        if (have && valid_match(g, b, i, j)) {
            const double4 q = w.pts[(int64_t)b * g.m + i];
            f = sampson_inlier(e, to_f4(q), t2);
            if (f) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // two-view depths: the point d0 (u0, v0, 1) whose image in camera 1 lies on the ray of (u1, v1, 1), least squares
                    const double* C = cand[k];
                    const double rx = C[0] * q.x + C[1] * q.y + C[2], ry = C[3] * q.x + C[4] * q.y + C[5], rz = C[6] * q.x + C[7] * q.y + C[8];
                    const double ax = q.w * rz - ry, ay = rx - q.z * rz, az = q.z * ry - q.w * rx;       // x1 x (R x0)
                    const double bx = q.w * C[11] - C[10], by = C[9] - q.z * C[11], bz = q.z * C[10] - q.w * C[9];   // x1 x t
                    const double d0 = -(ax * bx + ay * by + az * bz) / (ax * ax + ay * ay + az * az);
                    const double d1 = d0 * rz + C[11];
                    pos[k] += (d0 > 0.0 && d1 > 0.0);
                }
            }
        }
        inliers[(int64_t)b * g.m + i] = f ? 1 : 0;
        inl += f;
    }
    inl = block_sum(inl, red);
#pragma unroll
    for (int k = 0; k < 4; ++k) pos[k] = block_sum(pos[k], red);
    if (threadIdx.x != 0) return;
    num_inliers[b] = inl;
    if (!have) {
        error[b] = __builtin_huge_valf();
#pragma unroll
        for (int c = 0; c < 9; ++c) R_pred[b * 9 + c] = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) t_pred[b * 3 + c] = 0.0f;
        return;
    }
    int kb = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) kb = pos[k] > pos[kb] ? k : kb;
    const double* C = cand[kb];
    const float* Rt = g.R + b * 9; const float* Tt = g.T + b * 3;
    double tr = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) tr += (double)Rt[c] * C[c];
    const double rerr = fabs(acos(fmin(fmax((tr - 1.0) / 2.0, -1.0), 1.0)) * (180.0 / M_PI));
    const double nt = sqrt((double)Tt[0] * Tt[0] + (double)Tt[1] * Tt[1] + (double)Tt[2] * Tt[2]);
    const double np = sqrt(C[9] * C[9] + C[10] * C[10] + C[11] * C[11]);
    const double cs = (Tt[0] * C[9] + Tt[1] * C[10] + Tt[2] * C[11]) / fmax(nt * np, 1e-8);
    const double a = fabs(acos(fmin(fmax(cs, -1.0), 1.0)) * (180.0 / M_PI));
    const double terr = fmin(a, 180.0 - a);
    error[b] = (float)fmax(rerr, terr);
#pragma unroll
    for (int c = 0; c < 9; ++c) R_pred[b * 9 + c] = (float)C[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) t_pred[b * 3 + c] = (float)C[9 + c];
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int og_epipolar_precision(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                     const int64_t* matches0, const int32_t* num_keypoints0, const float* K0, const float* K1,
                                     const float* R, const float* T, double threshold, float* precision, float* matching_score,
                                     int32_t* num_correct, void* stream) {
    og_clear_status();
    if (batch <= 0 || m < 0 || n < 0 || !precision || !matching_score || !num_correct || !K0 || !K1 || !R || !T) return OG_E_INVALID;
    if (m > 0 && (!keypoints0 || !matches0 || (n > 0 && !keypoints1))) return OG_E_INVALID;
    const Geo g{keypoints0, keypoints1, matches0, num_keypoints0, K0, K1, R, T, batch, m, n};
    hipLaunchKernelGGL(precision_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, g, threshold, precision, matching_score, num_correct);
    return og_launch_status();
}

extern "C" int og_essential_5pt(int32_t count, const double* x0, const double* x1, double* E, int32_t* num_solutions, void* stream) {
    og_clear_status();
    if (count <= 0 || !x0 || !x1 || !E || !num_solutions) return OG_E_INVALID;
    SolveSrc src{};
    src.x0 = x0; src.x1 = x1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(solve_poly_kernel, dim3((count + kPolyLds - 1) / kPolyLds), dim3(kPolyLds), 0, st, src, count, E);
    hipLaunchKernelGGL(solve_roots_kernel, dim3((count + 255) / 256), dim3(256), 0, st, count, E, num_solutions);
    return og_launch_status();
}

extern "C" size_t og_relative_pose_workspace_bytes(int32_t batch, int32_t m, int32_t hypotheses) {
    if (batch <= 0 || m < 0 || hypotheses <= 0) return 0;
    return pose_bytes(batch, m, hypotheses);
}

extern "C" int og_relative_pose(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                const int64_t* matches0, const int32_t* num_keypoints0, const float* K0, const float* K1,
                                const float* R, const float* T, float ransac_threshold, int32_t hypotheses, uint64_t seed,
                                int64_t pair_offset, float* error, float* R_pred, float* t_pred, uint8_t* inliers,
                                int32_t* num_inliers, void* workspace_dev, void* stream) {
    og_clear_status();
    if (batch <= 0 || m < 0 || n < 0 || hypotheses <= 0 || (int64_t)hypotheses * kMaxSol > (1 << 30) ||
        (int64_t)batch * hypotheses > (1 << 30) || !K0 || !K1 || !R || !T || !error || !R_pred || !t_pred || !num_inliers ||
        !workspace_dev)
        return OG_E_INVALID;
    if (m > 0 && (!keypoints0 || !matches0 || !inliers || (n > 0 && !keypoints1))) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const Geo g{keypoints0, keypoints1, matches0, num_keypoints0, K0, K1, R, T, batch, m, n};
    PoseWs w = pose_layout(workspace_dev, batch, m, hypotheses);
    hipStream_t st = (hipStream_t)stream;
    const int count = batch * hypotheses;
    SolveSrc src{};
    src.pts = w.pts; src.idx = w.idx; src.cnt = w.count; src.m = m; src.H = hypotheses; src.seed = seed; src.pair_offset = pair_offset;
    hipLaunchKernelGGL(prep_kernel, dim3(batch), dim3(256), 0, st, g, ransac_threshold, w);
    hipLaunchKernelGGL(solve_poly_kernel, dim3((count + kPolyLds - 1) / kPolyLds), dim3(kPolyLds), 0, st, src, count, w.E);
    hipLaunchKernelGGL(solve_roots_kernel, dim3((count + 255) / 256), dim3(256), 0, st, count, w.E, w.nsol);
    const int groups = (hypotheses * kMaxSol + 255) / 256;
    hipLaunchKernelGGL(score_kernel, dim3(batch * groups), dim3(256), 0, st, w, m, hypotheses, groups);
    hipLaunchKernelGGL(finish_kernel, dim3(batch), dim3(256), 0, st, g, w, hypotheses, error, R_pred, t_pred, inliers, num_inliers);
    return og_launch_status();
}
