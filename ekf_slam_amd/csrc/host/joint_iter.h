// Fragment of abi.hip, a scan's pairings applied as ONE joint update, RELINEARISED (ekf_observe_model_joint_iterated / ekf_joint_iterate):
// joint_update.h's call with k_joint_factor_iter in k_joint_factor's place and a second record beside the first; and the loop that kernel
// runs, on the host with one lane.
#pragma once
namespace {
static_assert(EKF_JOINT_ITER_MAX == kJointIterMax && EKF_JOINT_ITER_MAX == EKF_MODEL_ITER_MAX, "the kernel's limit is the header's");
static_assert(EKF_JOINT_SUB_MAX == kJointSubMax, "the kernel's sub-state is the header's");

// the iteration record on the device and in pinned memory, at the first call
int32_t joint_iter_alloc(ekf_handle *h) {
    if (h->d_jiter) return EKF_OK;
    HIPCHK(h, halloc(h, &h->h_jiter, kJointIterRecordDoubles * sizeof(double), hipHostMallocDefault));
    HIPCHK(h, dalloc(h, &h->d_jiter, (size_t)kJointIterRecordDoubles));
    HIPCHK(h, hipDeviceSynchronize());                     // dalloc clears on the null stream (see removal_alloc)
    return EKF_OK;
}

void joint_iter_fill(const double *rec, ekf_joint_iter_result *it) {
    it->used = (int32_t)rec[0];
    it->converged = (int32_t)rec[1];
    it->last_step = rec[2];
    it->d2_last = rec[3];
    it->irregular_at = (int32_t)rec[4];
    it->irregular_obs = (int32_t)rec[5];
    it->ns = (int32_t)rec[6];
    it->reserved = 0;
    for (int k = 0; k < EKF_JOINT_SUB_MAX; ++k) it->x_sub[k] = rec[8 + k];
}
}  // namespace

extern "C" {
int32_t ekf_observe_model_joint_iterated(ekf_handle *h, const ekf_model_obs *obs, int64_t m, const int64_t *lm, double gate, int32_t iterations,
                                         double tol, ekf_joint_result *res, ekf_joint_iter_result *it, double *nu, double *S) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const JointIterCtl ctl = { iterations, tol, it };
    return observe_joint(h, "observe_model_joint_iterated: ", obs, m, lm, gate, &ctl, res, nu, S);
}

// The device's loop with ONE lane: device_math.h's texts in k_joint_factor_iter's order, on operands cut out of P_sub the way the kernel
// cuts them out of the state; then W = L^-1 H P_sub column by column in k_gather_joint's order, x' = x0 + W' y, P' = P_sub - W' W.
int32_t ekf_joint_iterate(const double *x_sub, const double *P_sub, const ekf_model_obs *obs, int64_t np_, int32_t iterations, double tol,
                          ekf_joint_iter_result *it, double *x_out, double *P_out) {
    if (!x_sub || !P_sub || !obs || !it || !x_out || !P_out || np_ < 1 || np_ > EKF_JOINT_MAX) return EKF_ERR_INVALID_ARG;
    if (iterations < 1 || iterations > EKF_JOINT_ITER_MAX || !(tol >= 0.0)) return EKF_ERR_INVALID_ARG;
    const int np = (int)np_, n = 2 * np, ns = 3 + n;
    constexpr int ld = kJointRows;
    std::vector<AssocModelEntry> e(np);
    for (int p = 0; p < np; ++p) {
        const ekf_model_obs &o = obs[p];
        if (o.model < EKF_MODEL_RANGE_BEARING || o.model > EKF_MODEL_RELATIVE_XY) return EKF_ERR_INVALID_ARG;
        const bool two = o.model == EKF_MODEL_RANGE_BEARING || o.model == EKF_MODEL_RELATIVE_XY;
        e[p] = AssocModelEntry();
        e[p].model = o.model;
        e[p].z[0] = o.z[0]; e[p].z[1] = two ? o.z[1] : 0.0;
        if (!std::isfinite(e[p].z[0]) || !std::isfinite(e[p].z[1])) return EKF_ERR_INVALID_ARG;
        if (two) {
            if (parse_R(o.R, e[p].R[0], e[p].R[1], e[p].R[2], e[p].R[3])) return EKF_ERR_INVALID_ARG;
        } else {
            if (!(std::isfinite(o.R[0]) && o.R[0] >= 0.0)) return EKF_ERR_INVALID_ARG;
            e[p].R[0] = o.R[0]; e[p].R[3] = 1.0;
        }
    }
    auto P = [&](int r, int c) { return r >= c ? P_sub[(size_t)c * ns + r] : P_sub[(size_t)r * ns + c]; };       // the lower triangle
    double prr[9];
    std::vector<double> strips(6 * np), diag3(3 * np), pab(4 * (np * (np - 1) / 2 + 1)), A((size_t)ld * ld), y(n), t(n), v(n), Hr(6 * np), Ht(4 * np),
        xi(x_sub, x_sub + ns), xn(ns), u(ns), dstep(ns);
    std::vector<int> posed(np);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) prr[3 * r + c] = P(r, c);
    for (int p = 0; p < np; ++p) {
        for (int tt = 0; tt < 3; ++tt) for (int r = 0; r < 2; ++r) strips[6 * p + 2 * tt + r] = P(3 + 2 * p + r, tt);
        diag3[3 * p] = P(3 + 2 * p, 3 + 2 * p); diag3[3 * p + 1] = P(4 + 2 * p, 3 + 2 * p); diag3[3 * p + 2] = P(4 + 2 * p, 4 + 2 * p);
        for (int b = 0; b < p; ++b)
            for (int q = 0; q < 4; ++q) pab[4 * (p * (p - 1) / 2 + b) + q] = P(3 + 2 * p + (q >> 1), 3 + 2 * b + (q & 1));
    }
    double rec[kJointIterRecordDoubles] = {};
    int used = 0, converged = 0, irr_at = -1, irr_obs = -1;
    double step = 0.0, d2_last = NAN;
    for (int i = 0;; ++i) {
        for (int p = 0; p < np; ++p) {
            double S[4], r[2];
            posed[p] = i == 0 ? ekfm::joint_pairing(e[p].model, e[p].z, e[p].R, prr, &strips[6 * p], &diag3[3 * p], x_sub, x_sub + 3 + 2 * p,
                                                    &Hr[6 * p], &Ht[4 * p], S, r)
                              : ekfm::joint_iter_pairing(e[p].model, e[p].z, e[p].R, prr, &strips[6 * p], &diag3[3 * p], x_sub, x_sub + 3 + 2 * p,
                                                         xi.data(), xi.data() + 3 + 2 * p, &Hr[6 * p], &Ht[4 * p], S, r);
            y[2 * p] = r[0]; y[2 * p + 1] = r[1];
            A[(2 * p) * ld + 2 * p] = S[0]; A[(2 * p) * ld + 2 * p + 1] = S[1];
            A[(2 * p + 1) * ld + 2 * p] = S[2]; A[(2 * p + 1) * ld + 2 * p + 1] = S[3];
        }
        for (int pa = 1; pa < np; ++pa)
            for (int pb = 0; pb < pa; ++pb) {
                double Sab[4];
                ekfm::joint_cross_block(&Hr[6 * pa], &Ht[4 * pa], &Hr[6 * pb], &Ht[4 * pb], prr, &strips[6 * pa], &strips[6 * pb],
                                        &pab[4 * (pa * (pa - 1) / 2 + pb)], Sab);
                for (int q = 0; q < 4; ++q) A[(2 * pa + (q >> 1)) * ld + 2 * pb + (q & 1)] = Sab[q];
            }
        int bad = np;
        for (int p = np - 1; p >= 0; --p)
            if (!posed[p]) bad = p;
        for (int k = 0; k < 2 * bad; ++k) {
            double lkk;
            if (!ekfm::joint_pivot(A[k * ld + k], lkk)) { bad = k >> 1; break; }
            ekfm::joint_factor_scale(A.data(), ld, y.data(), n, k, lkk, 0, 1);
            ekfm::joint_factor_update(A.data(), ld, y.data(), n, k, 0, 1);
        }
        if (bad < np) { irr_at = i; irr_obs = bad; break; }
        d2_last = 0.0;
        for (int p = 0; p < np; ++p) d2_last = ekfm::joint_prefix_add(d2_last, y[2 * p], y[2 * p + 1]);
        t = y;
        for (int k = n - 1; k >= 0; --k) ekfm::joint_back_step(A.data(), ld, t.data(), v.data(), k, 0, 1);
        ekfm::joint_iter_Htv(Hr.data(), Ht.data(), v.data(), np, u.data(), 0, 1);
        ekfm::joint_iter_move(prr, strips.data(), diag3.data(), pab.data(), np, x_sub, u.data(), xi.data(), xn.data(), dstep.data(), 0, 1);
        step = ekfm::joint_iter_step(dstep.data(), ns);
        used = i + 1;
        converged = step <= tol;
        if (converged || used == iterations) break;
        xi = xn;
    }
    rec[0] = used; rec[1] = converged; rec[2] = step; rec[3] = d2_last; rec[4] = irr_at; rec[5] = irr_obs; rec[6] = ns;
    for (int k = 0; k < ns; ++k) rec[8 + k] = irr_at < 0 ? xn[k] : xi[k];
    joint_iter_fill(rec, it);
    if (irr_at >= 0) {
        // all or nothing: the outputs are the inputs
        for (int k = 0; k < ns; ++k) x_out[k] = x_sub[k];
        for (size_t q = 0; q < (size_t)ns * ns; ++q) P_out[q] = P_sub[q];
        return EKF_OK;
    }
    // W(:, c) = L^-1 H P_sub(:, c), the robot's three terms before the landmark's two, then the chain in ascending j
    std::vector<double> W((size_t)n * ns);
    for (int c = 0; c < ns; ++c)
        for (int ii = 0; ii < n; ++ii) {
            const int p = ii >> 1, s = ii & 1;
            double acc = Hr[6 * p + 3 * s] * P(0, c);
            acc += Hr[6 * p + 3 * s + 1] * P(1, c);
            acc += Hr[6 * p + 3 * s + 2] * P(2, c);
            acc += Ht[4 * p + 2 * s] * P(3 + 2 * p, c);
            acc += Ht[4 * p + 2 * s + 1] * P(4 + 2 * p, c);
            for (int j = 0; j < ii; ++j) acc = acc - A[ii * ld + j] * W[(size_t)j * ns + c];
            W[(size_t)ii * ns + c] = acc / sqrt(A[ii * ld + ii]);
        }
    for (int c = 0; c < ns; ++c) {
        double xs = 0.0;
        for (int ii = 0; ii < n; ++ii) xs = xs + W[(size_t)ii * ns + c] * y[ii];
        x_out[c] = x_sub[c] + xs;
        for (int r = c; r < ns; ++r) {
            double d = 0.0;
            for (int ii = 0; ii < n; ++ii) d = d + W[(size_t)ii * ns + r] * W[(size_t)ii * ns + c];
            P_out[(size_t)c * ns + r] = P_out[(size_t)r * ns + c] = P(r, c) - d;
        }
    }
    return EKF_OK;
}
}  // extern "C"
