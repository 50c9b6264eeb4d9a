// Degree-trig / wrap / 2x2 inverse with the semantics the reference's MATLAB built-ins are documented to
// have at its call sites (cosd/sind: EKF_SLAM.m:42,58-59,63-64,84-88; atan2d/wrapTo360: EKF_SLAM.m:130,
// Correspondence.m:56; mpower(.,-1): EKF_SLAM.m:143).  Host+device so ekf_motion_model (host) and the
// kernels agree.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define EKF_MHD __host__ __device__ inline
#else
#define EKF_MHD inline
#endif

// These run on ONE wavefront in the latency chain of every update-step, where a taken-or-not branch costs more than both of its
// sides: value selections are marked unpredictable so that the compiler emits v_cndmask instead of exec-mask branches.
#if defined(__clang__)
#define EKF_SEL(c) __builtin_unpredictable(c)
#else
#define EKF_SEL(c) (c)
#endif

// A compiler-level fence, no instruction: what was read from memory before it is read again after it.  ekfm::model_iterate puts one at the
// top of its loop so that the 38 operands in LDS are re-read by each linearisation instead of being held in registers across all of them
// (held, k_gather_model_iter needs 323 registers and one workgroup fills a CU; re-read, an LDS load costs nothing beside the loop's divisions).
#define EKF_REREAD() __asm__ __volatile__("" ::: "memory")

namespace ekfm {

constexpr double kD2R = 0.017453292519943295;
constexpr double kR2D = 57.29577951308232;

// a (deg) = 90*n + r with r in [-45,45]; quad = n mod 4; n = round(a / 90), halves away from zero.
// No fmod: for |a| < 2^40 the quotient of an exact multiple of 90 is exact, 90*n is exactly representable and
// a - 90*n is exact (Sterbenz), so r (and exactness at multiples of 90 degrees) is the same as reducing
// mod 360 first -- and f64 fmod is by far the slowest thing in these kernels' scalar prologues.
// No division either (an f64 division is a ~15-instruction dependent sequence, and this runs twice in the latency chain of every
// update-step): n is first taken from a * (1/90), which is within one ulp of a / 90 and can therefore only be off by one
// where a / 90 is within an ulp of k + 1/2, i.e. where |r| comes out at or just beyond 45; r = a - 90 n is exact for either
// candidate, so ONE correction step restores exactly the n that round(a / 90) gives, ties (|r| == 45) included.
EKF_MHD void reduce90(double a, double &r, int &quad) {
    if (!(fabs(a) < 1099511627776.0)) a = fmod(a, 360.0);        // rare; Inf / NaN come out as NaN and stay NaN below
    const double q = a * (1.0 / 90.0);
    double n = copysign(floor(fabs(q) + 0.5), q);
    r = fma(-90.0, n, a);
    // round-half-away-from-zero of the TRUE quotient: r must lie in [-45, 45], and a tie goes to the larger |n|
    const bool up = (r > 45.0) | ((r == 45.0) & (a > 0.0)), down = (r < -45.0) | ((r == -45.0) & (a < 0.0));
    const double adj = EKF_SEL(up) ? 1.0 : (EKF_SEL(down) ? -1.0 : 0.0);
    n += adj;
    r = fma(-90.0, adj, r);                                       // exact (r -+ 90, or r itself)
    // n mod 4 without a 64-bit integer conversion: n - 4 floor(n / 4) is an exact double in {0, 1, 2, 3}
    quad = (int)(n - 4.0 * floor(n * 0.25));
}

// sin / cos on [-pi/4, pi/4] and atan on [0, inf): plain polynomial kernels instead of the libm routines.
// Why: every update-step carries two sincos and one atan2 on ONE lane in its dependent prologue; the device libm versions
// (general argument reduction, ~150 dependent instructions each) cost 1.3 us + 0.7 us of the ~7 us gather.  The argument
// is already reduced here (reduce90), so an odd / even minimax polynomial is all that is needed.  The same code runs on the
// host (ekf_motion_model), which therefore agrees with the kernels bit for bit.  Accuracy: < 1 ulp (sin, cos), < 2 ulp (atan)
// against glibc over 10^7 points (tests/test_abi_symbols.py::test_device_math_matches_libm runs the host build).
// Coefficients: the classic fdlibm minimax sets for sin / cos on [-pi/4, pi/4].
EKF_MHD double sin_pio4(double x) {
    const double z = x * x;
    double r = 1.58969099521155010221e-10;
    r = fma(r, z, -2.50507602534068634195e-08);
    r = fma(r, z, 2.75573137070700676789e-06);
    r = fma(r, z, -1.98412698298579493134e-04);
    r = fma(r, z, 8.33333333332248946124e-03);
    r = fma(r, z, -1.66666666666666324348e-01);
    return fma(x * z, r, x);
}

EKF_MHD double cos_pio4(double x) {
    const double z = x * x;
    double r = -1.13596475577881948265e-11;
    r = fma(r, z, 2.08757232129817482790e-09);
    r = fma(r, z, -2.75573143513906633035e-07);
    r = fma(r, z, 2.48015872894767294178e-05);
    r = fma(r, z, -1.38888888888741095749e-03);
    r = fma(r, z, 4.16666666666666019037e-02);
    // 1 - z/2 + z^2 r, with the rounding error of 1 - z/2 carried along (fdlibm's k_cos arrangement)
    const double hz = 0.5 * z, w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + z * (z * r));
}

// atan(t), t >= 0 finite or +inf.  t > 1 -> pi/2 - atan(1/t); then the nearest of the angles 0, pi/8, pi/4 is split off,
// atan(t) = k pi/8 + atan((t - c_k) / (1 + t c_k)), c_k = tan(k pi/8), leaving |u| <= tan(pi/16) = 0.199 for the odd
// Taylor series (12 terms: 0.199^25 / 25 < 2^-60).
EKF_MHD double atan_pos(double t) {
    const bool inv = t > 1.0;
    if (inv) t = 1.0 / t;                                   // +inf -> 0
    constexpr double kT8 = 0.41421356237309504880;          // tan(pi/8) = sqrt(2) - 1
    constexpr double kT16 = 0.19891236737965800691;         // tan(pi/16)
    constexpr double kT316 = 0.66817863791929891999;        // tan(3 pi/16)
    double base, u;
    if (t <= kT16) { base = 0.0; u = t; }
    else if (t <= kT316) { base = 0.39269908169872415481; u = (t - kT8) / fma(t, kT8, 1.0); }      // pi/8
    else { base = 0.78539816339744830962; u = (t - 1.0) / (t + 1.0); }                              // pi/4
    const double z = u * u;
    double r = 1.0 / 25.0;
    r = fma(r, z, -1.0 / 23.0);
    r = fma(r, z, 1.0 / 21.0);
    r = fma(r, z, -1.0 / 19.0);
    r = fma(r, z, 1.0 / 17.0);
    r = fma(r, z, -1.0 / 15.0);
    r = fma(r, z, 1.0 / 13.0);
    r = fma(r, z, -1.0 / 11.0);
    r = fma(r, z, 1.0 / 9.0);
    r = fma(r, z, -1.0 / 7.0);
    r = fma(r, z, 1.0 / 5.0);
    r = fma(r, z, -1.0 / 3.0);
    const double a = base + fma(u * z, r, u);
    return inv ? 1.57079632679489661923 - a : a;
}

// atan2 with the IEEE / MATLAB conventions for zeros, infinities and NaN
EKF_MHD double atan2_poly(double y, double x) {
    if (isnan(x) || isnan(y)) return NAN;
    const double ax = fabs(x), ay = fabs(y);
    double a;
    if (ay == 0.0) a = 0.0;                                  // atan2(+-0, x): 0 or pi
    else if (isinf(ax) && isinf(ay)) a = 0.78539816339744830962;
    else a = atan_pos(ay / ax);                              // ax == 0 -> +inf -> pi/2;  ax == inf -> 0
    if (signbit(x)) a = 3.14159265358979323846 - a;
    return copysign(a, y);
}

// exact at multiples of 90 degrees
EKF_MHD double sind(double a) {
    if (!isfinite(a)) return NAN;
    double r; int quad;
    reduce90(a, r, quad);
    const double t = kD2R * r;
    return quad == 0 ? sin_pio4(t) : quad == 1 ? cos_pio4(t) : quad == 2 ? -sin_pio4(t) : -cos_pio4(t);
}

EKF_MHD double cosd(double a) {
    if (!isfinite(a)) return NAN;
    double r; int quad;
    reduce90(a, r, quad);
    const double t = kD2R * r;
    return quad == 0 ? cos_pio4(t) : quad == 1 ? -sin_pio4(t) : quad == 2 ? -cos_pio4(t) : sin_pio4(t);
}

// sind and cosd of the same angle with one reduction and one sin/cos pair (non-finite angles give NaN through reduce90)
EKF_MHD void sincosd(double a, double &sn, double &cs) {
    double r; int quad;
    reduce90(a, r, quad);
    const double t = kD2R * r;
    const double s0 = sin_pio4(t), c0 = cos_pio4(t);
    // quad 0: (s, c)   1: (c, -s)   2: (-s, -c)   3: (-c, s)
    const double sa = EKF_SEL(quad & 1) ? c0 : s0, ca = EKF_SEL(quad & 1) ? s0 : c0;
    sn = EKF_SEL(quad & 2) ? -sa : sa;
    cs = EKF_SEL((quad + 1) & 2) ? -ca : ca;
}

EKF_MHD double atan2d(double y, double x) { return atan2_poly(y, x) * kR2D; }

// mod(a,360) with positive multiples of 360 mapped to 360 (Mapping Toolbox wrapTo360)
EKF_MHD double wrapTo360(double a) {
    if (!isfinite(a)) return NAN;
    // fast exact path for the usual range (one or two turns), fmod otherwise
    double w;
    if (a >= 0.0 && a < 720.0) w = a < 360.0 ? a : a - 360.0;     // exact
    else if (a < 0.0 && a >= -360.0) w = a;                       // == fmod(a,360) for |a| < 360
    else w = fmod(a, 360.0);
    if (w < 0.0) w += 360.0;
    if (w == 0.0 && a > 0.0) w = 360.0;
    return w;
}

// inverse of a 2x2 (row-major) the way inv() does it: LU with partial pivoting, no symmetry assumed.
// A singular phi yields inf/nan exactly as MATLAB's inv would (with a warning there).
EKF_MHD void inv2(const double a[4], double o[4]) {
    double p = a[0], q = a[1], r = a[2], t = a[3];
    const bool swap = fabs(r) > fabs(p);
    if (swap) { const double tp = p, tq = q; p = r; q = t; r = tp; t = tq; }
    const double l = r / p, u22 = t - l * q;
    const double i11 = 1.0 / p, i12 = -q / (p * u22), i22 = 1.0 / u22;
    const double m11 = i11 + i12 * (-l), m12 = i12, m21 = i22 * (-l), m22 = i22;
    if (swap) { o[0] = m12; o[1] = m11; o[2] = m22; o[3] = m21; }
    else      { o[0] = m11; o[1] = m12; o[2] = m21; o[3] = m22; }
}

// S = G H' + R of a constraint between landmarks i and j (constrain.h), from their own 2x2 blocks pii / pjj (lower-triangle entries
// (0,0) (1,0) (1,1)) and their cross block pij (row-major, P(a_i + r, a_j + b)); R and S row-major.  Written as
// G(:, a_i) - G(:, a_j) + R with G = P(a_i, :) - P(a_j, :), entry by entry -- the host (the singularity check, ekf_landmark_distance)
// and the kernel run this same function.
EKF_MHD void constrain_S(const double pii[3], const double pjj[3], const double pij[4], const double R[4], double S[4]) {
    for (int r = 0; r < 2; ++r)
        for (int b = 0; b < 2; ++b)
            S[2 * r + b] = ((pii[r + b] - pij[2 * b + r]) - (pij[2 * r + b] - pjj[r + b])) + R[2 * r + b];
}

// d2 = nu' S^-1 nu of that constraint (S row-major), the squared Mahalanobis distance a merge is gated on; returns whether S is
// regular (finite, S00 > 0, det S > 0) and leaves NaN in d2 where it is not.  The host (ekf_landmark_distance, the refusal of a singular
// constraint) and k_nearest (nearest.h) run this same function: with FP contraction off both give the same bits.
EKF_MHD bool constrain_d2(const double S[4], double nu0, double nu1, double &d2) {
    const double det = S[0] * S[3] - S[1] * S[2];
    const bool regular = isfinite(S[0]) && isfinite(S[1]) && isfinite(S[2]) && isfinite(S[3]) && S[0] > 0.0 && det > 0.0;
    double Si[4];
    inv2(S, Si);
    d2 = regular ? (nu0 * Si[0] + nu1 * Si[2]) * nu0 + (nu0 * Si[1] + nu1 * Si[3]) * nu1 : NAN;
    return regular;
}

// a (degrees) wrapped into (-180, 180]: a - 360 ceil((a - 180) / 360), the product exact and the difference one rounding
EKF_MHD double wrap180(double a) {
    if (a > -180.0 && a <= 180.0) return a;
    return fma(-360.0, ceil((a - 180.0) / 360.0), a);
}

// The small part of a LINEAR observation z = H x + noise (linear_obs.h), H = [Hr | Hl0 | Hl1] with a 2x3 block on the robot state and
// 2x2 blocks on up to two landmarks.  sm: the kLinearSmall operands, the 7 x 7 covariance of (robot, landmark 0, landmark 1) and their
// seven entries of x --
//   0..8    Prr, row-major                         9 + 6b + 2t + r   P(t, a_b + r): the strip at landmark b's columns
//   21 + 3b the own block of landmark b: (0,0) (1,0) (1,1)           27 + 2r + c   the cross block P(a_0 + r, a_1 + c)
//   31..33  x_r      34, 35  l_0      36, 37  l_1
// (an absent landmark: zeros, with a zero block of H).  H row-major 2 x 7, R and S row-major.  Gs = H Psm (2 x 7, row-major),
// S = Gs H' + R, nu = z - H x with the rows named in wrap_deg wrapped into (-180, 180], every sum in ascending index order.
// k_gather_linear, k_linear_probe and the host run this one function: with FP contraction off all give the same bits.
constexpr int kLinearSmall = 38;
EKF_MHD double linear_small_P(const double *sm, int i, int j) {
    if (i < j) { const int t = i; i = j; j = t; }
    if (i < 3) return sm[3 * i + j];
    const int b = (i - 3) >> 1, r = (i - 3) & 1;
    if (j < 3) return sm[9 + 6 * b + 2 * j + r];
    const int bj = (j - 3) >> 1, c = (j - 3) & 1;
    if (b == bj) return sm[21 + 3 * b + r + c];
    return sm[27 + 2 * c + r];                      // i in landmark 1, j in landmark 0: P(a_0 + c, a_1 + r)
}
EKF_MHD void linear_small(const double *sm, const double H[14], const double z[2], const double R[4], const int wrap_deg[2],
                          double Gs[14], double S[4], double nu[2]) {
    for (int r = 0; r < 2; ++r) {
        for (int j = 0; j < 7; ++j) {
            double g = 0.0;
            for (int i = 0; i < 7; ++i) g += H[7 * r + i] * linear_small_P(sm, i, j);
            Gs[7 * r + j] = g;
        }
        double hx = 0.0;
        for (int i = 0; i < 7; ++i) hx += H[7 * r + i] * sm[31 + i];
        nu[r] = z[r] - hx;
        if (wrap_deg[r]) nu[r] = wrap180(nu[r]);
    }
    for (int r = 0; r < 2; ++r)
        for (int b = 0; b < 2; ++b) {
            double s = 0.0;
            for (int j = 0; j < 7; ++j) s += Gs[7 * r + j] * H[7 * b + j];
            S[2 * r + b] = s + R[2 * r + b];
        }
}

// what a linear observation does under S, nu and its gate: EKF_LINEAR_IRREGULAR (0) where constrain_d2 calls S irregular (d2 is NaN),
// EKF_LINEAR_GATED (2) where d2 > gate, EKF_LINEAR_APPLIED (1) otherwise
EKF_MHD int linear_outcome(const double S[4], const double nu[2], double gate, double &d2) {
    if (!constrain_d2(S, nu[0], nu[1], d2)) return 0;
    return d2 > gate ? 2 : 1;
}

// The observation models of ekf_observe_model (include/ekfslam.h names them; model_obs.h runs them on the device): h(x) and its Jacobian
// H (row-major 2 x 7 over robot | landmark 0 | landmark 1, linear_small's layout) at xs = the seven entries sm[31..37].  The target t of
// models 1-4 is landmark 0 (has_landmark) or the fixed point `anchor`, which carries no block of H; model 5 is the distance between
// landmarks 0 and 1 and has no robot block.  theta in degrees, so a bearing's derivatives carry k = 180/pi and RELATIVE_XY's heading
// column 1/k.  A one-row model leaves row 1 of H and hx[1] exactly zero.  Returns whether q = |d|^2 is finite and positive; where it is
// not (the target on the robot, a non-finite state) H and hx are zero and the caller reports EKF_LINEAR_IRREGULAR.
// Each expression is written once: the host (ekf_model_evaluate), k_model_probe and k_gather_model give the same bits.
EKF_MHD bool model_eval(int model, const double xs[7], const double anchor[2], bool has_landmark, double hx[2], double H[14]) {
    for (int i = 0; i < 14; ++i) H[i] = 0.0;
    hx[0] = hx[1] = 0.0;
    const bool pair = model == 5;
    const double tx = pair || has_landmark ? xs[3] : anchor[0], ty = pair || has_landmark ? xs[4] : anchor[1];
    const double px = pair ? xs[5] : xs[0], py = pair ? xs[6] : xs[1];
    const double dx = tx - px, dy = ty - py;
    const double q = dx * dx + dy * dy;
    if (!(isfinite(q) && q > 0.0) || !isfinite(xs[2])) return false;
    const double r = sqrt(q);
    const int tcol = 3, pcol = pair ? 5 : 0;                    // where the blocks on t and on p go
    const bool tblock = pair || has_landmark;
    if (model == 1 || model == 2 || model == 5) {               // row 0: the range
        const double ex = dx / r, ey = dy / r;
        hx[0] = r;
        H[pcol] = -ex; H[pcol + 1] = -ey;
        if (tblock) { H[tcol] = ex; H[tcol + 1] = ey; }
    }
    if (model == 1 || model == 3) {                             // the bearing: row 1 of RANGE_BEARING, row 0 of BEARING
        const int row = model == 1 ? 7 : 0;
        const double bx = kR2D * dy / q, by = kR2D * dx / q;
        hx[model == 1 ? 1 : 0] = atan2d(dy, dx) - xs[2];
        H[row] = bx; H[row + 1] = -by; H[row + 2] = -1.0;
        if (tblock) { H[row + tcol] = -bx; H[row + tcol + 1] = by; }
    }
    if (model == 4) {                                           // the target in the robot frame
        double s, c;
        sincosd(xs[2], s, c);
        hx[0] = c * dx + s * dy;
        hx[1] = c * dy - s * dx;
        H[0] = -c; H[1] = -s; H[2] = hx[1] / kR2D;
        H[7] = s; H[8] = -c; H[9] = -hx[0] / kR2D;
        if (tblock) { H[3] = c; H[4] = s; H[10] = -s; H[11] = c; }
    }
    return true;
}
// which rows of a model's nu are angles in degrees, wrapped into (-180, 180]
EKF_MHD void model_wrap(int model, int wrap_deg[2]) {
    wrap_deg[0] = model == 3;
    wrap_deg[1] = model == 1;
}

// The small part of a MODEL observation: linear_small with nu = z - h(x) in place of z - H x (rows wrapped as model_wrap says); Gs and S
// in linear_small's summation order, so a linear observation handed this H gives the same Gs and S bit for bit.  Kept beside
// linear_small, not split out of it: k_gather_linear's registers are pinned.  (The two meet one level up: each is what
// the small_solve overload of its argument block runs, linear_obs.h / model_obs.h.)
EKF_MHD void model_small(const double *sm, const double H[14], const double hx[2], const double z[2], const double R[4],
                         const int wrap_deg[2], double Gs[14], double S[4], double nu[2]) {
    for (int r = 0; r < 2; ++r) {
        for (int j = 0; j < 7; ++j) {
            double g = 0.0;
            for (int i = 0; i < 7; ++i) g += H[7 * r + i] * linear_small_P(sm, i, j);
            Gs[7 * r + j] = g;
        }
        nu[r] = z[r] - hx[r];
        if (wrap_deg[r]) nu[r] = wrap180(nu[r]);
    }
    for (int r = 0; r < 2; ++r)
        for (int b = 0; b < 2; ++b) {
            double s = 0.0;
            for (int j = 0; j < 7; ++j) s += Gs[7 * r + j] * H[7 * b + j];
            S[2 * r + b] = s + R[2 * r + b];
        }
}

// The ITERATED small part of a model observation (ekf_observe_model_iterated; model_iter.h runs it on lane 0): Gauss-Newton on the MAP
// cost over the seven entries x0 = sm[31..37] under their 7 x 7 covariance P in sm, relinearising h up to `iterations` times --
//     xi_0 = x0;   (h_i, H_i) at xi_i;   Gs_i = H_i P;   S_i = Gs_i H_i' + R       (model_small: its sums, its order)
//     r_i = wrap(z - h_i) - H_i (x0 - xi_i)     (i = 0: wrap(z - h_0) alone, no second term formed)
//     xi_{i+1} = x0 + Gs_i' S_i^-1 r_i;   step = max_k |xi_{i+1}[k] - xi_i[k]|;   stop after i = iterations - 1 or where step <= tol
// The GATE is read at the first linearisation only: outcome0 / d2_0 / S_0 / nu_0 are ekf_model_innovation's, and a first linearisation
// that does not apply ends the loop with used = 0.  A later iterate that is not posed (model_eval false) or whose S is irregular
// (constrain_d2) makes the whole call EKF_LINEAR_IRREGULAR, all or nothing: used = the linearisations whose step was taken.
// `converged` is step <= tol, so under tol = 0 a step of exactly 0 (a model that is linear in effect) counts as converged and stops.
// H, Gs, S and r are the LAST linearisation's, the operands of the pair; xi is xi_used, the seven entries the pair leaves in x.
// With iterations = 1 model_eval, model_wrap, model_small and linear_outcome run in model_obs.h's order: the same bits.
constexpr int kModelIterMax = 16;
struct ModelIterate {
    double S0[4], nu0[2], d2;      // the first linearisation's, what the 8-double record reports
    double xi[7];
    double last_step;
    int used, converged;
};
EKF_MHD int model_iterate(int model, const double *sm, const double anchor[2], bool has_landmark, const double z[2], const double R[4],
                          double gate, int iterations, double tol, double H[14], double Gs[14], double S[4], double r[2], ModelIterate &it) {
    double hx[2], xi[7];
    int wrap[2];
    model_wrap(model, wrap);
    for (int k = 0; k < 7; ++k) xi[k] = sm[31 + k];
    it.last_step = 0.0;
    it.used = it.converged = 0;
    int outcome = 1;
    for (int i = 0; i < iterations; ++i) {
        EKF_REREAD();
        const bool posed = model_eval(model, xi, anchor, has_landmark, hx, H);
        model_small(sm, H, hx, z, R, wrap, Gs, S, r);
        if (i == 0) {
            outcome = linear_outcome(S, r, gate, it.d2);
            if (!posed) { outcome = 0; it.d2 = NAN; }
            for (int q = 0; q < 4; ++q) it.S0[q] = S[q];
            it.nu0[0] = r[0]; it.nu0[1] = r[1];
        } else {
            for (int q = 0; q < 2; ++q) {
                double hd = 0.0;
                for (int k = 0; k < 7; ++k) hd += H[7 * q + k] * (sm[31 + k] - xi[k]);
                r[q] -= hd;
            }
            double d2i;
            if (!posed || !constrain_d2(S, r[0], r[1], d2i)) outcome = 0;
        }
        if (outcome != 1) break;
        double Si[4], step = 0.0;
        inv2(S, Si);
        for (int k = 0; k < 7; ++k) {
            const double k0 = Gs[k] * Si[0] + Gs[7 + k] * Si[2], k1 = Gs[k] * Si[1] + Gs[7 + k] * Si[3];
            const double nx = sm[31 + k] + (k0 * r[0] + k1 * r[1]);
            step = fmax(step, fabs(nx - xi[k]));
            xi[k] = nx;
        }
        it.last_step = step;
        it.used = i + 1;
        it.converged = step <= tol;
        if (it.converged) break;
    }
    for (int k = 0; k < 7; ++k) it.xi[k] = xi[k];
    return outcome;
}

// The INVERSE of the two models that determine a point (ekf_append_model; append_model.h runs it on the device): the landmark t = g(x_r, z)
// that z observes from the pose xr, with Gx = dg/dx_r (row-major 2 x 3) and Gz = dg/dz (row-major 2 x 2).  Gx is always [1 0 gth0; 0 1 gth1]:
// only gth = dg/dtheta depends on the state.  theta and a bearing in degrees, k = 180/pi, as in model_eval -- so H_t Gz = I and
// H_r + H_t Gx = 0 with model_eval's blocks at (xr, t).  RANGE_BEARING z = (r, b): t = p + r (cosd, sind)(theta + b); RELATIVE_XY
// z = (a, b): t = p + Rot(theta) z.  Returns false (nothing written) for any other model.  Each expression is written once: the host
// (ekf_model_invert) and k_append_model give the same bits.
EKF_MHD bool model_invert(int model, const double xr[3], const double z[2], double t[2], double gth[2], double Gz[4]) {
    if (model == 1) {
        double s, c;
        sincosd(xr[2] + z[1], s, c);
        t[0] = xr[0] + z[0] * c;
        t[1] = xr[1] + z[0] * s;
        gth[0] = -z[0] * s / kR2D;
        gth[1] = z[0] * c / kR2D;
        Gz[0] = c; Gz[1] = gth[0];
        Gz[2] = s; Gz[3] = gth[1];
        return true;
    }
    if (model == 4) {
        double s, c;
        sincosd(xr[2], s, c);
        const double w0 = c * z[0] - s * z[1], w1 = s * z[0] + c * z[1];
        t[0] = xr[0] + w0;
        t[1] = xr[1] + w1;
        gth[0] = -w1 / kR2D;
        gth[1] = w0 / kR2D;
        Gz[0] = c; Gz[1] = -s;
        Gz[2] = s; Gz[3] = c;
        return true;
    }
    return false;
}

// ekf_associate_model (associate_model.h runs it on the device, one lane per landmark): d2 of one observation through a model whose target
// is ONE landmark, from the live F64 copies alone -- prr (row-major), the strip at the landmark's columns (strip6[2 t + r] = P(t, a + r)),
// its own block diag3 ((0,0) (1,0) (1,1)), the pose xr and the landmark l.  The kLinearSmall operands are laid out exactly as
// linear_small_entry fills them for a = {2 i, -1} (landmark 1 absent: zeros) and go through model_eval, model_wrap, model_small and
// constrain_d2 -- no shortened form, the zero terms included: the sums are k_model_probe's, so d2 is ekf_model_innovation's bit for bit.
// Returns whether the pair has a d2 (the target off the robot, the state finite, S regular); d2 is NaN where it has none.
EKF_MHD bool assoc_model_d2(int model, const double z[2], const double R[4], const double prr[9], const double strip6[6],
                            const double diag3[3], const double xr[3], const double l[2], double &d2) {
    double sm[kLinearSmall];
    for (int e = 0; e < kLinearSmall; ++e) sm[e] = 0.0;
    for (int e = 0; e < 9; ++e) sm[e] = prr[e];
    for (int e = 0; e < 6; ++e) sm[9 + e] = strip6[e];
    for (int e = 0; e < 3; ++e) { sm[21 + e] = diag3[e]; sm[31 + e] = xr[e]; }
    sm[34] = l[0]; sm[35] = l[1];
    const double anchor[2] = { 0.0, 0.0 };
    double H[14], hx[2], Gs[14], S[4], nu[2];
    int wrap[2];
    const bool posed = model_eval(model, sm + 31, anchor, true, hx, H);
    model_wrap(model, wrap);
    model_small(sm, H, hx, z, R, wrap, Gs, S, nu);
    const bool regular = constrain_d2(S, nu[0], nu[1], d2);
    if (!posed) d2 = NAN;
    return posed && regular && !isnan(d2);
}

// The two best landmarks of a scan's observation and the two counts beside them (ekf_model_match's fields, in its order): the record a lane,
// a wavefront, a workgroup and the whole grid hold alike.  Candidates are ordered by (d2, index): smaller d2 first, the lower index on equal
// d2; index -1 is "none" (d2 = +inf) and comes after every candidate.
struct Match2 {
    long long best, second;
    double d2_best, d2_second;
    long long within, irregular;
};
EKF_MHD void match2_init(Match2 &m) {
    m.best = m.second = -1;
    m.d2_best = m.d2_second = INFINITY;
    m.within = m.irregular = 0;
}
EKF_MHD bool match2_before(double d2a, long long ia, double d2b, long long ib) {
    return ia >= 0 && (ib < 0 || d2a < d2b || (d2a == d2b && ia < ib));
}
// one candidate into the top two
EKF_MHD void match2_insert(Match2 &m, double d2, long long i) {
    const bool first = match2_before(d2, i, m.d2_best, m.best), second = match2_before(d2, i, m.d2_second, m.second);
    if (first) { m.d2_second = m.d2_best; m.second = m.best; m.d2_best = d2; m.best = i; }
    else if (second) { m.d2_second = d2; m.second = i; }
}
// landmark i with its d2 (regular: it has one): a candidate, counted where d2 <= gate; otherwise counted as irregular and never a candidate
EKF_MHD void match2_offer(Match2 &m, double d2, long long i, bool regular, double gate) {
    if (!regular) { m.irregular += 1; return; }
    if (d2 <= gate) m.within += 1;
    match2_insert(m, d2, i);
}
// the top two of the union and the counts added: associative and commutative (the order is total and no index occurs twice), so every
// reduction shape gives the same record
EKF_MHD Match2 match2_merge(const Match2 &a, const Match2 &b) {
    Match2 r = a;
    match2_insert(r, b.d2_best, b.best);
    match2_insert(r, b.d2_second, b.second);
    r.within += b.within;
    r.irregular += b.irregular;
    return r;
}

// The MOTION models of ekf_predict_model (include/ekfslam.h names them; predict_model.h runs them on the device): the new pose
// xn = f(x_r, u), the two entries fa = F(0,2), fb = F(1,2) of F = df/dx_r = I + [0 0 fa; 0 0 fb; 0 0 0], and V = df/du (row-major 3 x 3; a
// model with two inputs leaves column 2 zero).  theta, the turn and V's heading row in degrees, so the heading column of F and the turn
// column of V carry 1/k, k = 180/pi.  The new heading is wrapTo360(theta + turn) as ekf_predict forms it; sincosd is taken of the unwrapped
// sums.  fa, fb and V depend on theta and u alone, never on the position.
//   1 TURN_DRIVE  u = (d, t):      turn by t, then drive d -- the reference's own f (EKF_SLAM.m:58-60), with its true Jacobians
//   2 ARC         u = (d, t):      the circular arc of length d that turns by t, in chord form: chord d g along theta + t/2, g = sin a / a,
//                                  a = t / (2k); finite at t = 0 (g, g' = dg/da from their series below kMotionSeries)
//   3 POSE_DELTA  u = (dx, dy, t): the pose increment in the robot frame (a scan matcher, integrated odometry)
// Returns false (nothing written) for any other model.  The sincos is a parameter because the kernels keep ONE machine-code body of it
// (predict.h: sincosd_ni); each expression is written once, so the host (ekf_motion_evaluate), the host emulation and k_predict_model
// give the same bits with FP contraction off.
constexpr double kMotionSeries = 0.5;
// g(a) = sin a / a and g'(a) = (a cos a - sin a) / a^2 given sin a and cos a.  Below kMotionSeries the closed form of g' cancels (its
// relative error grows as 3 eps / a^2) and both are 0 / 0 at a = 0: there the Taylor series, cut where the next term is below half an ulp
// at the switch (g: a^16 / 17! = 4e-20; g': 16 a^15 / 17! = 1.4e-18 against 0.16).
EKF_MHD void motion_chord(double a, double sa, double ca, double &g, double &gp) {
    if (fabs(a) < kMotionSeries) {
        const double z = a * a;
        double r = 1.0 / 1307674368000.0;                       // 1 / 15!
        r = fma(r, z, -1.0 / 6227020800.0);                     // 1 / 13!
        r = fma(r, z, 1.0 / 39916800.0);
        r = fma(r, z, -1.0 / 362880.0);
        r = fma(r, z, 1.0 / 5040.0);
        r = fma(r, z, -1.0 / 120.0);
        r = fma(r, z, 1.0 / 6.0);
        g = fma(-z, r, 1.0);
        double q = -14.0 / 1307674368000.0;                     // -2n / (2n + 1)!, n = 7 .. 1
        q = fma(q, z, 12.0 / 6227020800.0);
        q = fma(q, z, -10.0 / 39916800.0);
        q = fma(q, z, 8.0 / 362880.0);
        q = fma(q, z, -6.0 / 5040.0);
        q = fma(q, z, 4.0 / 120.0);
        q = fma(q, z, -2.0 / 6.0);
        gp = a * q;
    } else {
        g = sa / a;
        gp = (a * ca - sa) / (a * a);
    }
}
struct MotionSinCos {
    EKF_MHD void operator()(double a, double &sn, double &cs) const { sincosd(a, sn, cs); }
};
template <typename SinCos>
EKF_MHD bool motion_eval_with(const SinCos &sc, int model, const double xr[3], const double u[3], double xn[3], double &fa, double &fb,
                              double V[9]) {
    if (model < 1 || model > 3) return false;
    for (int i = 0; i < 9; ++i) V[i] = 0.0;
    double s, c;
    if (model == 3) {
        sc(xr[2], s, c);
        const double w0 = c * u[0] - s * u[1], w1 = s * u[0] + c * u[1];
        xn[0] = xr[0] + w0;
        xn[1] = xr[1] + w1;
        xn[2] = wrapTo360(xr[2] + u[2]);
        fa = -w1 / kR2D;
        fb = w0 / kR2D;
        V[0] = c; V[1] = -s;
        V[3] = s; V[4] = c;
        V[8] = 1.0;
        return true;
    }
    double dg = u[0], g = 1.0, gp = 0.0;                       // the chord and what it is of the arc
    if (model == 2) {
        const double half = 0.5 * u[1], a = half / kR2D;
        double sa, ca;
        sc(half, sa, ca);
        motion_chord(a, sa, ca, g, gp);
        dg = u[0] * g;
        sc(xr[2] + half, s, c);
    } else {
        sc(xr[2] + u[1], s, c);
    }
    xn[0] = xr[0] + dg * c;                                     // EKF_SLAM.m:58-60 where model == 1
    xn[1] = xr[1] + dg * s;
    xn[2] = wrapTo360(xr[2] + u[1]);
    fa = -dg * s / kR2D;
    fb = dg * c / kR2D;
    if (model == 2) {
        V[0] = g * c; V[1] = u[0] * (gp * c - g * s) / (2.0 * kR2D);
        V[3] = g * s; V[4] = u[0] * (gp * s + g * c) / (2.0 * kR2D);
    } else {
        V[0] = c; V[1] = fa;
        V[3] = s; V[4] = fb;
    }
    V[7] = 1.0;
    return true;
}
EKF_MHD bool motion_eval(int model, const double xr[3], const double u[3], double xn[3], double &fa, double &fb, double V[9]) {
    return motion_eval_with(MotionSinCos(), model, xr, u, xn, fa, fb, V);
}
// the turn of a step: the entry of u that the heading takes up
EKF_MHD double motion_turn(int model, const double u[3]) { return model == 3 ? u[2] : u[1]; }
// entry (i, j) of Q = V M V' (V row-major 3 x 3, M symmetric from its lower triangle m6 = (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)): T = V M, then
// T V', both sums in ascending index order, the zero terms of a two-input model included
EKF_MHD double motion_M(const double m6[6], int r, int c) {
    if (r < c) { const int t = r; r = c; c = t; }
    return m6[r * (r + 1) / 2 + c];
}
EKF_MHD double motion_noise_entry(const double V[9], const double m6[6], int i, int j) {
    double q = 0.0;
    for (int k = 0; k < 3; ++k) {
        double t = 0.0;
        for (int l = 0; l < 3; ++l) t += V[3 * i + l] * motion_M(m6, l, k);
        q += t * V[3 * j + k];
    }
    return q;
}

// JOINT compatibility of a scan's pairings (ekf_joint_innovation; joint.h runs these on the device): observation k paired with landmark
// l_k for every paired k, the rows stacked -- S = H P H' + blockdiag(R_k), d2 = nu' S^-1 nu.
// One pairing: assoc_model_d2's operands through the same model_eval, model_wrap and model_small, so S (row-major) and nu are
// ekf_model_innovation's for that pair bit for bit; what the off-diagonal blocks need of H is left in Hr (row-major 2 x 3, the robot block)
// and Ht (row-major 2 x 2, the target's).  Returns whether the pair is posed (model_eval).
EKF_MHD bool joint_pairing(int model, const double z[2], const double R[4], const double prr[9], const double strip6[6], const double diag3[3],
                           const double xr[3], const double l[2], double Hr[6], double Ht[4], double S[4], double nu[2]) {
    double sm[kLinearSmall];
    for (int e = 0; e < kLinearSmall; ++e) sm[e] = 0.0;
    for (int e = 0; e < 9; ++e) sm[e] = prr[e];
    for (int e = 0; e < 6; ++e) sm[9 + e] = strip6[e];
    for (int e = 0; e < 3; ++e) { sm[21 + e] = diag3[e]; sm[31 + e] = xr[e]; }
    sm[34] = l[0]; sm[35] = l[1];
    const double anchor[2] = { 0.0, 0.0 };
    double H[14], hx[2], Gs[14];
    int wrap[2];
    const bool posed = model_eval(model, sm + 31, anchor, true, hx, H);
    model_wrap(model, wrap);
    model_small(sm, H, hx, z, R, wrap, Gs, S, nu);
    for (int r = 0; r < 2; ++r) {
        for (int t = 0; t < 3; ++t) Hr[3 * r + t] = H[7 * r + t];
        for (int c = 0; c < 2; ++c) Ht[2 * r + c] = H[7 * r + 3 + c];
    }
    return posed;
}
// The 2 x 2 block S_ab (row-major) of two pairings a != b on different landmarks:
//     S_ab = Har (Prr Hbr' + strip_b Hbt') + Hat (strip_a' Hbr' + Pab Hbt')
// prr row-major (read from its lower triangle, as linear_small_P does), strip_x[2 t + r] = P(t, l_x + r), pab[2 r + c] = P(l_a + r, l_b + c).
// Every sum in ascending index order, the robot's terms before the landmark's; the host build of the tests compiles this same text.
EKF_MHD void joint_cross_block(const double Har[6], const double Hat[4], const double Hbr[6], const double Hbt[4], const double prr[9],
                               const double strip_a[6], const double strip_b[6], const double pab[4], double Sab[4]) {
    double M1[6], M2[4];                            // M1 = Prr Hbr' + strip_b Hbt' (3 x 2), M2 = strip_a' Hbr' + Pab Hbt' (2 x 2)
    for (int t = 0; t < 3; ++t)
        for (int j = 0; j < 2; ++j) {
            double v = 0.0;
            for (int u = 0; u < 3; ++u) v += (t >= u ? prr[3 * t + u] : prr[3 * u + t]) * Hbr[3 * j + u];
            for (int c = 0; c < 2; ++c) v += strip_b[2 * t + c] * Hbt[2 * j + c];
            M1[2 * t + j] = v;
        }
    for (int r = 0; r < 2; ++r)
        for (int j = 0; j < 2; ++j) {
            double v = 0.0;
            for (int t = 0; t < 3; ++t) v += strip_a[2 * t + r] * Hbr[3 * j + t];
            for (int c = 0; c < 2; ++c) v += pab[2 * r + c] * Hbt[2 * j + c];
            M2[2 * r + j] = v;
        }
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            double v = 0.0;
            for (int t = 0; t < 3; ++t) v += Har[3 * i + t] * M1[2 * t + j];
            for (int r = 0; r < 2; ++r) v += Hat[2 * i + r] * M2[2 * r + j];
            Sab[2 * i + j] = v;
        }
}
// The right-looking Cholesky factorisation of the n x n matrix A (lower triangle, leading dimension ld) with the forward substitution
// riding along: y enters as nu and leaves as L^-1 nu, being one more row of A below the last.  Step k is a pivot, a column scale and a
// trailing update, each entry's terms subtracted in ascending k -- so L's (and y's) leading part depends on A's leading block alone, with
// the same bits whatever follows.  Written per lane: lane `lane` of `lanes` takes every lanes-th entry of a step's phase, the phases
// separated by the caller (a barrier on the device; the host runs them with one lane).
EKF_MHD bool joint_pivot(double p, double &lkk) {
    lkk = sqrt(p);
    return isfinite(p) && p > 0.0;
}
EKF_MHD void joint_factor_scale(double *A, int ld, double *y, int n, int k, double lkk, int lane, int lanes) {
    for (int i = k + 1 + lane; i <= n; i += lanes) {
        if (i < n) A[i * ld + k] = A[i * ld + k] / lkk;
        else y[k] = y[k] / lkk;
    }
}
EKF_MHD void joint_factor_update(double *A, int ld, double *y, int n, int k, int lane, int lanes) {
    const int w = n - k - 1;                        // trailing rows; entry e < w * w: (i, j) = k + 1 + (e / w, e % w), the lower triangle kept
    for (int e = lane; e < w * w + w; e += lanes) {
        if (e < w * w) {
            const int i = k + 1 + e / w, j = k + 1 + e % w;
            if (j <= i) A[i * ld + j] = A[i * ld + j] - A[i * ld + k] * A[j * ld + k];
        } else {
            const int i = k + 1 + (e - w * w);
            y[i] = y[i] - A[i * ld + k] * y[k];
        }
    }
}
// a pairing's two rows added to the running d2, in row order
EKF_MHD double joint_prefix_add(double acc, double y0, double y1) {
    acc = acc + y0 * y0;
    return acc + y1 * y1;
}
// The ROW-APPEND of that factorisation (ekf_joint_search; joint_search.h runs these on the device): a hypothesis is its parent plus one
// pairing, so its factor is the parent's with the two rows i0, i0 + 1 appended, in O(i0^2) where a factorisation from scratch costs
// O(i0^3).  L (leading dimension ld) is the parent's factor with the PIVOT'S ROOT l_kk on its diagonal (joint_factor_* leave l_kk^2 there),
// y its L^-1 nu.  The two rows enter in a0 / a1 as their S entries -- a0[0 .. i0], a1[0 .. i0 + 1] -- each with its nu behind its diagonal
// entry (a0[i0 + 1], a1[i0 + 2]), and leave in l0 / l1 laid out alike: L's entries, the pivot's root on the diagonal, then y.  Every entry
// sees the operations joint_factor_scale / joint_factor_update apply to it, in their order -- a = a - L_ik L_jk for ascending k, then
// a / l_jj -- so L, y and every prefix are the right-looking factorisation's bit for bit.  Step k < i0, lane `lane` of `lanes`, the steps
// separated by the caller (a barrier); l0 / l1 do not alias a0 / a1 (a step's divisor a[k] is read by every lane).
EKF_MHD void joint_append_step(const double *L, int ld, const double *y, double *a0, double *a1, double *l0, double *l1, int i0, int k,
                               int lane, int lanes) {
    const double lkk = L[k * ld + k];
    const double e0 = a0[k] / lkk, e1 = a1[k] / lkk;
    if (lane == 0) { l0[k] = e0; l1[k] = e1; }
    for (int j = k + 1 + lane; j <= i0 + 2; j += lanes) {
        if (j < i0) {
            const double ljk = L[j * ld + k];
            a0[j] = a0[j] - e0 * ljk;
            a1[j] = a1[j] - e1 * ljk;
        } else if (j == i0) {                       // row i0's diagonal; row i0 + 1 against row i0
            a0[j] = a0[j] - e0 * e0;
            a1[j] = a1[j] - e1 * e0;
        } else if (j == i0 + 1) {                   // row i0's y; row i0 + 1's diagonal
            a0[j] = a0[j] - e0 * y[k];
            a1[j] = a1[j] - e1 * e1;
        } else {                                    // row i0 + 1's y
            a1[j] = a1[j] - e1 * y[k];
        }
    }
}
// ... and the close, by ONE lane behind the last step: row i0's pivot and y, step i0 of row i0 + 1, its pivot and y.  False where a pivot
// fails joint_pivot: the pairing is irregular and nothing of l0 / l1 is to be read.
EKF_MHD bool joint_append_close(const double *a0, double *a1, double *l0, double *l1, int i0) {
    double lkk;
    if (!joint_pivot(a0[i0], lkk)) return false;
    l0[i0] = lkk;
    const double y0 = a0[i0 + 1] / lkk;
    l0[i0 + 1] = y0;
    const double e1 = a1[i0] / lkk;
    l1[i0] = e1;
    a1[i0 + 1] = a1[i0 + 1] - e1 * e1;
    a1[i0 + 2] = a1[i0 + 2] - e1 * y0;
    if (!joint_pivot(a1[i0 + 1], lkk)) return false;
    l1[i0 + 1] = lkk;
    l1[i0 + 2] = a1[i0 + 2] / lkk;
    return true;
}
// The ORDER of a joint-compatibility search's survivors: more pairings first, then the smaller joint d2, then the hypothesis, compared
// entry by entry in scan order on the 0-based landmark with -1 for left out -- Python's order of the tuples (-pairings, d2, hypothesis).
// A hypothesis is given as its parent's n entries and its own last one.  No d2 here is NaN (a NaN does not survive its test).
EKF_MHD bool joint_search_before(int pa, double da, const long long *ha, long long ta, int pb, double db, const long long *hb, long long tb,
                                 int n) {
    if (pa != pb) return pa > pb;
    if (da != db) return da < db;
    for (int k = 0; k < n; ++k)
        if (ha[k] != hb[k]) return ha[k] < hb[k];
    return ta < tb;
}
// an extension's test: NaN never survives
EKF_MHD bool joint_search_passes(double d2, double threshold) { return d2 <= threshold; }
// the cut: how many of `survived` stay alive under `beam`, and whether that is a cut -- exactly `beam` survivors is none
EKF_MHD int joint_search_cut(int survived, int beam, bool &truncated) {
    truncated = survived > beam;
    return truncated ? beam : survived;
}

// The ITERATED joint update (ekf_observe_model_joint_iterated; joint_iter.h runs these on the device, ekf_joint_iterate on the host with
// one lane): Gauss-Newton on the MAP cost over the sub-state xi = (x_r, l_0 .. l_{np-1}), ns = 3 + 2 np entries, under its PRIOR covariance
//     P_sub = [Prr, the strip columns of the paired landmarks; their own blocks; the blocks P(l_a, l_b)]
// kept as the operands joint_pairing and joint_cross_block read: prr (row-major, its lower triangle read), strips[6 p + 2 t + r] =
// P(t, l_p + r), diag3[3 p ..] = P(l_p, l_p)'s (0,0) (1,0) (1,1), pab[4 (a (a - 1) / 2 + b) + 2 r + c] = P(l_a + r, l_b + c) for a > b.
//     xi_0 = x0;   (H_i, nu_i = wrap(z - h(xi_i))) per pairing, S_i = H_i P_sub H_i' + R from the PRIOR operands (joint_pairing,
//     joint_cross_block: their sums, their order);   r_i = nu_i - H_i (x0 - xi_i)   (i = 0: nu_0 alone, no second term formed)
//     L_i L_i' = S_i, y_i = L_i^-1 r_i (joint_factor_*);   v = L_i^-T y_i (joint_back_step);   u = H_i' v (joint_iter_Htv)
//     xi_{i+1} = x0 + P_sub u (joint_iter_move);   step = max_k |xi_{i+1}[k] - xi_i[k]| (joint_iter_step)
// The move is the back-substitution form, O(ns^2): the other form, W_sub' y_i with the full W_sub = L_i^-1 H_i P_sub, costs O(ns^3) and a
// second ns x 2 np array on-die for a vector that is needed once per linearisation.
// P_sub(k, j), k, j < ns:
EKF_MHD double joint_sub_P(const double prr[9], const double *strips, const double *diag3, const double *pab, int k, int j) {
    if (k < j) { const int t = k; k = j; j = t; }              // the lower triangle: k >= j
    if (k < 3) return prr[3 * k + j];
    const int pa = (k - 3) >> 1, ra = (k - 3) & 1;
    if (j < 3) return strips[6 * pa + 2 * j + ra];
    const int pb = (j - 3) >> 1, rb = (j - 3) & 1;
    if (pa == pb) return diag3[3 * pa + ra + rb];              // (0,0) (1,0) (1,1)
    return pab[4 * (pa * (pa - 1) / 2 + pb) + 2 * ra + rb];
}
// One pairing of linearisation i >= 1: joint_pairing at (xir, xil) with the prior operands, then the residual r = nu - H (x0 - xi), the
// robot's three terms before the landmark's two, each row's sum formed before it is subtracted (model_iterate's order).
EKF_MHD bool joint_iter_pairing(int model, const double z[2], const double R[4], const double prr[9], const double strip6[6], const double diag3[3],
                                const double x0r[3], const double x0l[2], const double xir[3], const double xil[2], double Hr[6], double Ht[4],
                                double S[4], double r[2]) {
    const bool posed = joint_pairing(model, z, R, prr, strip6, diag3, xir, xil, Hr, Ht, S, r);
    for (int q = 0; q < 2; ++q) {
        double hd = 0.0;
        for (int t = 0; t < 3; ++t) hd += Hr[3 * q + t] * (x0r[t] - xir[t]);
        for (int c = 0; c < 2; ++c) hd += Ht[2 * q + c] * (x0l[c] - xil[c]);
        r[q] -= hd;
    }
    return posed;
}
// Step k = n - 1 .. 0 of v = L^-T t on the factored A (strict lower triangle L, the pivot L_kk^2 on the diagonal, as joint_factor_* leave
// it): v[k] = t[k] / L_kk, then t[i] loses L(k, i) v[k] for every i < k -- so entry i's terms are subtracted in DESCENDING k.  Every lane
// forms v[k] itself from t[k], which the step before finished; lane 0 stores it.  One phase a step, the caller separates the steps.
EKF_MHD void joint_back_step(const double *A, int ld, double *t, double *v, int k, int lane, int lanes) {
    const double vk = t[k] / sqrt(A[k * ld + k]);
    if (lane == 0) v[k] = vk;
    for (int i = lane; i < k; i += lanes) t[i] = t[i] - A[k * ld + i] * vk;
}
// u = H' v over the sub-state: the robot's entry t sums over the pairings in ascending row order, a landmark's entry over its own two rows
EKF_MHD void joint_iter_Htv(const double *Hr, const double *Ht, const double *v, int np, double *u, int lane, int lanes) {
    for (int k = lane; k < 3 + 2 * np; k += lanes) {
        double s = 0.0;
        if (k < 3) {
            for (int i = 0; i < 2 * np; ++i) s += Hr[6 * (i >> 1) + 3 * (i & 1) + k] * v[i];
        } else {
            const int p = (k - 3) >> 1, c = (k - 3) & 1;
            for (int q = 0; q < 2; ++q) s += Ht[4 * p + 2 * q + c] * v[2 * p + q];
        }
        u[k] = s;
    }
}
// xn = x0 + P_sub u, entry k's sum in ascending j and added to x0[k] last; dstep[k] = |xn[k] - xi[k]|
EKF_MHD void joint_iter_move(const double prr[9], const double *strips, const double *diag3, const double *pab, int np, const double *x0,
                             const double *u, const double *xi, double *xn, double *dstep, int lane, int lanes) {
    const int ns = 3 + 2 * np;
    for (int k = lane; k < ns; k += lanes) {
        double s = 0.0;
        for (int j = 0; j < ns; ++j) s += joint_sub_P(prr, strips, diag3, pab, k, j) * u[j];
        xn[k] = x0[k] + s;
        dstep[k] = fabs(xn[k] - xi[k]);
    }
}
// the largest move, in ascending k (fmax: a NaN entry is passed over, as in model_iterate); every lane reads the same ns entries
EKF_MHD double joint_iter_step(const double *dstep, int ns) {
    double step = 0.0;
    for (int k = 0; k < ns; ++k) step = fmax(step, dstep[k]);
    return step;
}

}  // namespace ekfm
