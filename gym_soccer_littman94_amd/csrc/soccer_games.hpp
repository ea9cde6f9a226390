// soccer_games.hpp — exact solution of a 5x5 zero-sum matrix game in float64 (the stage game of minimax value
// iteration, Shapley 1953 / Littman 1994).  Plain portable C++: IEEE + - * /, fabs and comparisons only, so the
// same source compiles for the GPU (hipcc) and for the host (g++, tests/host/games_host.cpp), and with
// -ffp-contract=off on both sides the two builds return the same bits.
//
// A[a * 5 + b] is the row player's (A's, the maximiser's) payoff.  solve_game5 returns the value v, a maximin
// strategy x of the row player and a minimax strategy y of the column player:
//   * pure saddle point (max_a min_b A == min_b max_a A): a* = first row whose minimum is the max-min, b* = first
//     column whose maximum is the min-max; v = A[a*][b*] bit for bit, x = e_a*, y = e_b*.  Exact.  (returns 1)
//   * otherwise the simplex method on the game's LP, with Bland's rule (terminates on degenerate games) and a hard
//     bound on the pivots.  The matrix is shifted and scaled into [1, 2] so that the LP is bounded and feasible at
//     the slack basis.  x and y are the LP's dual and primal solutions, clipped at 0 and renormalised.  (returns 0)
//   * every mixed answer is VERIFIED before it is returned: with the bracket the strategies certify on the caller's
//     matrix,  lo = min_b (x^T A)_b <= value <= hi = max_a (A y)_a,  it is accepted only when hi - lo <= eps.  A simplex
//     answer that fails (near-ties and ill-conditioned bases end the pivoting on a basis that is optimal only to the
//     pivot tolerance) is replaced by Shapley-Snow enumeration: the square submatrices in a fixed order (support size
//     1..5, then row and column subsets in ascending bit order; 251 candidates), each solved for both players'
//     equalising strategies by Gaussian elimination with partial pivoting, the first candidate that passes the same
//     check is returned.  (returns 2; should no candidate pass, the narrowest bracket seen is returned, returns 3)
//   v is the midpoint of the accepted bracket.
// Accuracy contract (eps = 1e-10 * max(1, max|A|)): min_b (x^T A)_b >= v - eps, max_a (A y)_a <= v + eps,
// x, y >= 0, sum x = sum y = 1 within 1e-12.  Accepting at width eps, half of what the contract allows, leaves the
// rest for the rounding of whoever recomputes the bracket.
//
// The tableau and the candidates live in caller memory (GameWork): they are indexed with run-time row and column
// numbers, which in a kernel's private array would put them in scratch; a kernel hands each solver an LDS slot.
// Everything else uses compile-time indices only.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SOCCER_GAME_HD __host__ __device__
#define SOCCER_GAME_UNROLL _Pragma("unroll")
#else
#define SOCCER_GAME_HD
#define SOCCER_GAME_UNROLL
#endif

namespace soccer {

constexpr int kGameN = 5;
constexpr int kGameCols = 2 * kGameN + 1;         // 5 structural, 5 slack, right-hand side
constexpr int kGameMaxPivots = 64;                // Bland's rule needs no more than a handful; C(10, 5) = 252 bases in all

struct GameWork {
    double t[kGameN + 1][kGameCols];              // rows 0..4 constraints, row 5 the objective (reduced costs)
    double x[kGameN], y[kGameN];                  // the strategies under test
    double bx[kGameN], by[kGameN];                // the narrowest bracket so far (enumeration)
    int basis[kGameN];                            // column index of the basic variable of each row
    int sub[2][kGameN];                           // a candidate's rows and columns
};

// the bracket (x, y) certify on A:  lo = min_b (x^T A)_b,  hi = max_a (A y)_a
SOCCER_GAME_HD inline void game_bracket(const double* A, const double* x, const double* y, double* lo, double* hi) {
    constexpr int N = kGameN;
    double l = 0.0, h = 0.0;
    SOCCER_GAME_UNROLL
    for (int b = 0; b < N; ++b) {
        double s = 0.0;
        SOCCER_GAME_UNROLL
        for (int a = 0; a < N; ++a) s = s + x[a] * A[a * N + b];
        l = (b == 0 || s < l) ? s : l;
    }
    SOCCER_GAME_UNROLL
    for (int a = 0; a < N; ++a) {
        double s = 0.0;
        SOCCER_GAME_UNROLL
        for (int b = 0; b < N; ++b) s = s + A[a * N + b] * y[b];
        h = (a == 0 || s > h) ? s : h;
    }
    *lo = l; *hi = h;
}

// clip at 0 and renormalise in place; false when nothing positive is left
SOCCER_GAME_HD inline bool game_normalise(double* z) {
    double sum = 0.0;
    SOCCER_GAME_UNROLL
    for (int i = 0; i < kGameN; ++i) { z[i] = z[i] > 0.0 ? z[i] : 0.0; sum = sum + z[i]; }
    if (!(sum > 0.0)) return false;
    SOCCER_GAME_UNROLL
    for (int i = 0; i < kGameN; ++i) z[i] = z[i] / sum;
    return true;
}

// The equalising strategy of one player on the k x k submatrix (rows sub[0][..], columns sub[1][..]) of
// B = (A - lo) * inv + 1:  COL = false solves  sum_i z_i B[I_i][J_r] = w (r < k), sum_i z_i = 1  for the row player,
// COL = true the transposed system for the column player; z is written to out[] (zeros off the support).
// Gaussian elimination with partial pivoting on the augmented (k+1) x (k+2) system in w->t.  false: singular.
SOCCER_GAME_HD inline bool game_equalise(const double* A, GameWork* w, int k, bool col, double lo, double inv, double* out) {
    constexpr int N = kGameN;
    double (*m)[kGameCols] = w->t;
    const int n = k + 1;
    for (int r = 0; r < k; ++r) {
        for (int c = 0; c < k; ++c) {
            const int a = col ? w->sub[0][r] : w->sub[0][c], b = col ? w->sub[1][c] : w->sub[1][r];
            m[r][c] = (A[a * N + b] - lo) * inv + 1.0;
        }
        m[r][k] = -1.0; m[r][n] = 0.0;
    }
    for (int c = 0; c < k; ++c) m[k][c] = 1.0;
    m[k][k] = 0.0; m[k][n] = 1.0;
    for (int c = 0; c < n; ++c) {
        int pr = c;
        for (int r = c + 1; r < n; ++r) if (fabs(m[r][c]) > fabs(m[pr][c])) pr = r;
        if (m[pr][c] == 0.0) return false;
        if (pr != c) for (int j = c; j <= n; ++j) { const double tmp = m[c][j]; m[c][j] = m[pr][j]; m[pr][j] = tmp; }
        for (int r = c + 1; r < n; ++r) {
            const double f = m[r][c] / m[c][c];
            if (f == 0.0) continue;
            for (int j = c; j <= n; ++j) m[r][j] = m[r][j] - f * m[c][j];
        }
    }
    for (int r = n - 1; r >= 0; --r) {
        double s = m[r][n];
        for (int j = r + 1; j < n; ++j) s = s - m[r][j] * m[j][n];
        m[r][n] = s / m[r][r];
    }
    for (int i = 0; i < N; ++i) out[i] = 0.0;
    for (int c = 0; c < k; ++c) out[w->sub[col ? 1 : 0][c]] = m[c][n];
    return true;
}

// 1 = pure saddle point, 0 = simplex, 2 = Shapley-Snow enumeration, 3 = no candidate passed (narrowest bracket)
SOCCER_GAME_HD inline int solve_game5(const double* A, GameWork* w, double* v_out, double* x, double* y) {
    constexpr int N = kGameN;
    // ---- pure saddle point ------------------------------------------------------------------------------
    double maxmin = 0.0, minmax = 0.0;
    int astar = 0, bstar = 0;
    SOCCER_GAME_UNROLL
    for (int a = 0; a < N; ++a) {
        double m = A[a * N];
        SOCCER_GAME_UNROLL
        for (int b = 1; b < N; ++b) m = A[a * N + b] < m ? A[a * N + b] : m;
        if (a == 0 || m > maxmin) { maxmin = m; astar = a; }
    }
    SOCCER_GAME_UNROLL
    for (int b = 0; b < N; ++b) {
        double m = A[b];
        SOCCER_GAME_UNROLL
        for (int a = 1; a < N; ++a) m = A[a * N + b] > m ? A[a * N + b] : m;
        if (b == 0 || m < minmax) { minmax = m; bstar = b; }
    }
    if (maxmin == minmax) {
        double v = 0.0;
        SOCCER_GAME_UNROLL
        for (int a = 0; a < N; ++a) {
            SOCCER_GAME_UNROLL
            for (int b = 0; b < N; ++b) if (a == astar && b == bstar) v = A[a * N + b];
        }
        if (v_out) *v_out = v;
        SOCCER_GAME_UNROLL
        for (int i = 0; i < N; ++i) {
            if (x) x[i] = i == astar ? 1.0 : 0.0;
            if (y) y[i] = i == bstar ? 1.0 : 0.0;
        }
        return 1;
    }
    // ---- simplex on  max sum q  s.t.  B q <= 1, q >= 0,  B = (A - lo) / (hi - lo) + 1 in [1, 2] ----------
    // (hi > lo here: a constant matrix has a saddle point.)  At the optimum sum q = 1 / val(B), y = q / sum q, and
    // the reduced costs of the slacks are the dual p with x = p / sum p.
    double lo = A[0], hi = A[0];
    SOCCER_GAME_UNROLL
    for (int i = 1; i < N * N; ++i) { lo = A[i] < lo ? A[i] : lo; hi = A[i] > hi ? A[i] : hi; }
    const double range = hi - lo;
    double (*t)[kGameCols] = w->t;
    SOCCER_GAME_UNROLL
    for (int a = 0; a < N; ++a) {
        SOCCER_GAME_UNROLL
        for (int b = 0; b < N; ++b) t[a][b] = (A[a * N + b] - lo) / range + 1.0;
        SOCCER_GAME_UNROLL
        for (int c = 0; c < N; ++c) t[a][N + c] = a == c ? 1.0 : 0.0;
        t[a][2 * N] = 1.0;
        w->basis[a] = N + a;
    }
    SOCCER_GAME_UNROLL
    for (int c = 0; c < 2 * N + 1; ++c) t[N][c] = c < N ? -1.0 : 0.0;
    constexpr double tol = 1e-12;                 // entries of the scaled tableau are O(1)
    for (int it = 0; it < kGameMaxPivots; ++it) {
        int col = -1;                             // Bland: the lowest-index column with a negative reduced cost
        for (int c = 0; c < 2 * N && col < 0; ++c) if (t[N][c] < -tol) col = c;
        if (col < 0) break;
        int row = -1; double best = 0.0;          // minimum ratio, ties to the lowest basic-variable index (Bland)
        for (int r = 0; r < N; ++r) {
            const double piv = t[r][col];
            if (!(piv > tol)) continue;
            const double ratio = t[r][2 * N] / piv;
            if (row < 0 || ratio < best || (ratio == best && w->basis[r] < w->basis[row])) { row = r; best = ratio; }
        }
        if (row < 0) break;                       // unbounded: impossible for B > 0, kept as a guard
        const double piv = t[row][col];
        for (int c = 0; c < 2 * N + 1; ++c) t[row][c] = t[row][c] / piv;
        t[row][col] = 1.0;
        for (int r = 0; r < N + 1; ++r) {
            if (r == row) continue;
            const double f = t[r][col];
            if (f == 0.0) continue;
            for (int c = 0; c < 2 * N + 1; ++c) t[r][c] = t[r][c] - f * t[row][c];
            t[r][col] = 0.0;
        }
        w->basis[row] = col;
    }
    // strategies: clip at 0, renormalise
    double sq = 0.0, sp = 0.0;
    SOCCER_GAME_UNROLL
    for (int b = 0; b < N; ++b) {
        double val = 0.0;
        SOCCER_GAME_UNROLL
        for (int r = 0; r < N; ++r) if (w->basis[r] == b) val = t[r][2 * N];
        w->y[b] = val > 0.0 ? val : 0.0;
        sq = sq + w->y[b];
    }
    SOCCER_GAME_UNROLL
    for (int a = 0; a < N; ++a) {
        const double val = t[N][N + a];
        w->x[a] = val > 0.0 ? val : 0.0;
        sp = sp + w->x[a];
    }
    SOCCER_GAME_UNROLL
    for (int i = 0; i < N; ++i) {
        w->y[i] = sq > 0.0 ? w->y[i] / sq : 1.0 / N;
        w->x[i] = sp > 0.0 ? w->x[i] / sp : 1.0 / N;
    }
    // verify: accept the simplex answer only when the bracket it certifies is at most eps wide
    const double amax = hi > -lo ? hi : -lo;
    const double eps = 1e-10 * (amax > 1.0 ? amax : 1.0);
    double lo_c = 0.0, hi_c = 0.0;
    game_bracket(A, w->x, w->y, &lo_c, &hi_c);
    int path = 0;
    if (!(hi_c - lo_c <= eps)) {
        // Shapley-Snow: the first square submatrix whose equalising strategies pass the same check
        path = 3;
        double best = 0.0;
        bool have = false;
        const double inv = 1.0 / range;
        for (int k = 1; k <= N && path == 3; ++k) {
            for (int rm = 1; rm < (1 << N) && path == 3; ++rm) {
                int nr = 0;
                for (int i = 0; i < N; ++i) if (rm & (1 << i)) w->sub[0][nr++] = i;
                if (nr != k) continue;
                for (int cm = 1; cm < (1 << N) && path == 3; ++cm) {
                    int nc = 0;
                    for (int i = 0; i < N; ++i) if (cm & (1 << i)) w->sub[1][nc++] = i;
                    if (nc != k) continue;
                    if (!game_equalise(A, w, k, false, lo, inv, w->x) || !game_equalise(A, w, k, true, lo, inv, w->y)) continue;
                    if (!game_normalise(w->x) || !game_normalise(w->y)) continue;
                    double l = 0.0, h = 0.0;
                    game_bracket(A, w->x, w->y, &l, &h);
                    if (h - l <= eps) { lo_c = l; hi_c = h; path = 2; break; }
                    if (h - l == h - l && (!have || h - l < best)) {        // (not NaN) the narrowest so far
                        have = true; best = h - l;
                        for (int i = 0; i < N; ++i) { w->bx[i] = w->x[i]; w->by[i] = w->y[i]; }
                    }
                }
            }
        }
        if (path == 3) {                                            // nothing passed: the narrowest bracket seen
            for (int i = 0; i < N; ++i) { w->x[i] = have ? w->bx[i] : 1.0 / N; w->y[i] = have ? w->by[i] : 1.0 / N; }
            game_bracket(A, w->x, w->y, &lo_c, &hi_c);
        }
    }
    if (v_out) *v_out = 0.5 * (lo_c + hi_c);
    SOCCER_GAME_UNROLL
    for (int i = 0; i < N; ++i) {
        if (x) x[i] = w->x[i];
        if (y) y[i] = w->y[i];
    }
    return path;
}

}  // namespace soccer
