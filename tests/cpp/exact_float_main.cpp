// The keep rule of the exact search's fp16 list pass (auncel_amd/csrc/exact_args.h: exact_float_constant / _bound / _slack / _keep, the
// definitions scan_all_f16_kernel compiles) checked on the host, as a program of its own:
//   g++ -std=c++17 -g -O1 -ffp-contract=off tests/cpp/exact_float_main.cpp -o exact_float_main
// (add -fsanitize=address,undefined -fno-sanitize-recover=all for the sanitizers).
// For pairs of fp32 rows at d = 8, 30, 96, 128 and both metrics -- Gaussian rows, the same at the largest and the smallest magnitudes
// the scale rule admits, a row as tiny beside the largest as the rule admits, integer rows up to 2048 (held exactly: the smaller
// constant), the all-zero pair and a zero query -- it computes the reference's distance r with its own four running sums, rounds the
// operands to fp16 under the matrices' scales, accumulates the dot product of the halves in fp32 in three orders (forward, reversed,
// pairwise: the matrix cores promise no order) and requires that the rule KEEPS the pair for a threshold of exactly r and for one
// ulp on the keeping side of r.  How many pairs it keeps one per cent on the rejecting side is printed, not judged: that is the work
// the rescoring gets, not a matter of correctness.  Prints DONE and returns 0 when every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../auncel_amd/csrc/exact_args.h"

using namespace amdivf;

static long failures = 0;

// round to nearest even into fp16's grid (normal numbers: 11 significant bits; below 2^-14: multiples of 2^-24), as a float
static float to_half(float v) {
    if (v == 0.f) return v;
    const float a = std::fabs(v);
    float r;
    if (a < 6.103515625e-05f) {
        r = std::nearbyint(a * 16777216.f) / 16777216.f;
    } else {
        int e;
        const float mant = std::frexp(a, &e);  // a = mant 2^e, mant in [0.5, 1)
        r = std::ldexp(std::nearbyint(mant * 2048.f), e - 11);
    }
    return v < 0 ? -r : r;
}

// the reference's distance: running sums 0..3 over elements 4 i + l, products and sums rounded separately, (s0 + s1) + (s2 + s3)
static float reference(bool l2, const float* x, const float* y, int dpad) {
    volatile float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < dpad; c++) {
        volatile float t;
        if (l2) {
            volatile float df = y[c] - x[c];
            t = df * df;
        } else {
            t = y[c] * x[c];
        }
        s[c & 3] = s[c & 3] + t;
    }
    volatile float a = s[0] + s[1], b = s[2] + s[3];
    return a + b;
}

static float norm_of(bool l2, const float* x, int d) {
    double sq = 0.0;
    for (int c = 0; c < d; c++) sq += (double)x[c] * (double)x[c];
    return l2 ? (float)sq : (float)std::sqrt(sq);
}

struct Matrix {
    int rows, d, dpad;
    std::vector<float> v;  // rows x dpad, zero beyond d
    const float* row(int r) const { return v.data() + (size_t)r * dpad; }
    float* row(int r) { return v.data() + (size_t)r * dpad; }
};

// the scale rule (ivf_filter.hip: half_scale_of): 1 where every element is an integer of magnitude <= 2048, else the power of two that
// brings the largest magnitude into [2^14, 2^15); exact: the former
static float scale_of(const Matrix& m, bool& exact) {
    float amax = 0.f;
    exact = true;
    for (float x : m.v) {
        amax = std::fmax(amax, std::fabs(x));
        exact &= x == (float)(int)x && std::fabs(x) <= 2048.f;
    }
    if (exact || amax == 0.f) return 1.f;
    int e;
    (void)std::frexp(amax, &e);
    return std::ldexp(1.f, 15 - e);
}

static float pairwise(const std::vector<float>& t, size_t lo, size_t hi) {
    if (hi - lo == 1) return t[lo];
    const size_t mid = lo + (hi - lo) / 2;
    volatile float a = pairwise(t, lo, mid), b = pairwise(t, mid, hi);
    return a + b;
}

static long pairs_seen = 0, kept_beyond = 0;

static void check_pairs(bool l2, const Matrix& X, const Matrix& Y, const char* what) {
    bool ex, ey;
    const float sx = scale_of(X, ex), sy = scale_of(Y, ey);
    const float C = exact_float_constant(X.d, ex && ey), ps = 1.f / (sx * sy);
    std::vector<float> hx(X.dpad), hy(X.dpad), prod(X.dpad);
    for (int i = 0; i < X.rows; i++) {
        const float xn = norm_of(l2, X.row(i), X.d);
        for (int c = 0; c < X.dpad; c++) hx[c] = to_half(X.row(i)[c] * sx);
        for (int j = 0; j < Y.rows; j++) {
            const float yn = norm_of(l2, Y.row(j), Y.d);
            const float r = reference(l2, X.row(i), Y.row(j), X.dpad);
            for (int c = 0; c < X.dpad; c++) {
                hy[c] = to_half(Y.row(j)[c] * sy);
                prod[c] = hx[c] * hy[c];  // (two halves: exact in fp32)
            }
            volatile float fwd = 0.f, rev = 0.f;
            for (int c = 0; c < X.dpad; c++) fwd = fwd + prod[c];
            for (int c = X.dpad - 1; c >= 0; c--) rev = rev + prod[c];
            const float sums[3] = {fwd, rev, pairwise(prod, 0, prod.size())};
            // the keeping side of r: a larger threshold under L2, a smaller one under the inner product
            const float keep_side = std::nextafter(r, l2 ? INFINITY : -INFINITY);
            const float beyond = l2 ? r - 0.01f * std::fabs(r) : r + 0.01f * std::fabs(r);
            for (float sum : sums) {
                const float p = ps * sum;
                for (float tau : {r, keep_side}) {
                    const bool keep = exact_float_keep(l2, C, p, yn, exact_float_bound(l2, C, xn, tau), exact_float_slack(l2, C, xn));
                    if (!keep) {
                        if (failures < 20)
                            printf("FAILED %s %s d %d pair (%d, %d): r %a tau %a p %a xn %a yn %a C %a\n", what, l2 ? "L2" : "IP", X.d, i, j, r, tau, p, xn,
                                   yn, C);
                        failures++;
                    }
                }
                if (beyond != r) {
                    pairs_seen++;
                    kept_beyond += exact_float_keep(l2, C, p, yn, exact_float_bound(l2, C, xn, beyond), exact_float_slack(l2, C, xn));
                }
            }
        }
    }
}

static Matrix gaussian(std::mt19937& g, int rows, int d, float mul) {
    Matrix m{rows, d, (d + 3) & ~3, {}};
    m.v.assign((size_t)rows * m.dpad, 0.f);
    std::normal_distribution<float> n(0.f, 1.f);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < d; c++) m.row(r)[c] = n(g) * mul;
    return m;
}
static Matrix integers(std::mt19937& g, int rows, int d, int top) {
    Matrix m = gaussian(g, rows, d, 0.f);
    std::uniform_int_distribution<int> u(-top, top);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < d; c++) m.row(r)[c] = (float)u(g);
    return m;
}
static float amax_of(const Matrix& m) {
    float a = 0.f;
    for (float x : m.v) a = std::fmax(a, std::fabs(x));
    return a;
}
// multiplies the matrix by the power of two that puts its largest magnitude into [2^(e-1), 2^e)
static void to_exponent(Matrix& m, int e) {
    int have;
    (void)std::frexp(amax_of(m), &have);
    for (float& x : m.v) x = std::ldexp(x, e - have);
}
// row r halved until its largest element is as near 2^-12 of the matrix's as a power of two brings it from above: the smallest
// the scale rule admits
static void tiny_row(Matrix& m, int r) {
    const float limit = amax_of(m) * 0.000244140625f;
    float rmax = 0.f;
    for (int c = 0; c < m.d; c++) rmax = std::fmax(rmax, std::fabs(m.row(r)[c]));
    float f = 1.f;
    while (rmax * f * 0.5f >= limit) f *= 0.5f;
    for (int c = 0; c < m.d; c++) m.row(r)[c] *= f;
}

int main() {
    std::mt19937 g(12345);
    const int NQ = 8, NY = 48;
    for (int d : {8, 30, 96, 128})
        for (int metric = 0; metric < 2; metric++) {
            const bool l2 = metric == 1;
            {
                Matrix X = gaussian(g, NQ, d, 1.f), Y = gaussian(g, NY, d, 1.f);
                check_pairs(l2, X, Y, "gaussian");
                // near neighbours: the distance is small beside the norms, where the bound is widest beside the value
                Matrix Z = Y;
                for (int i = 0; i < NQ; i++)
                    for (int c = 0; c < d; c++) Z.row(i)[c] = X.row(i)[c] * (1.f + 0.001f * (float)c);
                check_pairs(l2, X, Z, "near");
                Matrix Xl = X, Yl = Y, Xs = X, Ys = Y;
                to_exponent(Xl, 24), to_exponent(Yl, 24), to_exponent(Xs, -24), to_exponent(Ys, -24);
                check_pairs(l2, Xl, Yl, "largest magnitudes");
                check_pairs(l2, Xs, Ys, "smallest magnitudes");
                check_pairs(l2, Xl, Ys, "largest against smallest");
                Matrix Xt = X, Yt = Y;
                tiny_row(Xt, 1), tiny_row(Yt, 2), tiny_row(Yt, 5);
                check_pairs(l2, Xt, Yt, "tiny rows");
            }
            {
                Matrix X = integers(g, NQ, d, 2048), Y = integers(g, NY, d, 2048);
                check_pairs(l2, X, Y, "integers to 2048");
                Matrix Xs = integers(g, NQ, d, 8), Ys = integers(g, NY, d, 8);
                check_pairs(l2, Xs, Ys, "integers to 8");
                check_pairs(l2, Xs, gaussian(g, NY, d, 1.f), "integers against gaussian");
            }
            {
                Matrix X = gaussian(g, NQ, d, 1.f), Y = gaussian(g, NY, d, 1.f);
                for (int c = 0; c < d; c++) X.row(0)[c] = Y.row(0)[c] = Y.row(7)[c] = 0.f;  // the all-zero pair, a zero query, zero vectors
                check_pairs(l2, X, Y, "zero rows");
                Matrix X0 = gaussian(g, 1, d, 0.f), Y0 = gaussian(g, 2, d, 0.f);
                check_pairs(l2, X0, Y0, "all zero");
                check_pairs(l2, X0, Y, "zero queries only");
            }
        }
    printf("kept %ld of %ld (pair, order) tests at a threshold one per cent on the rejecting side (information)\n", kept_beyond, pairs_seen);
    if (failures) {
        printf("%ld FAILED\n", failures);
        return 1;
    }
    printf("DONE\n");
    return 0;
}
