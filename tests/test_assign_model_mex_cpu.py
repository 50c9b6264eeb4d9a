"""CPU: the MEX gateway's `assign_model` command under the MEX mock with a recording stand-in for ekf_assign_model, the gateway linked
against a stand-in that lacks the symbol, and the MATLAB methods that forward to the command."""
import os
import re

from mex_harness import ROOT, driver, driver_without, prelude, transcript_of

# ` out0=MxN[...]` ... ` out3=...`: as many outputs as the command was asked for
SHOWN4 = prelude(r'''    for (int k = 0; k < nlhs && k < 4; ++k)
        if (out[k] && mxGetClassID(out[k]) != mxUINT64_CLASS) {
            printf(" out%d=%zux%zu[", k, mxGetM(out[k]), mxGetN(out[k]));
            for (size_t i = 0; i < mxGetM(out[k]) * mxGetN(out[k]); ++i) printf(i ? ",%g" : "%g", mxGetPr(out[k])[i]);
            printf("]");
        }
''')

_STUB = r'''
#include <math.h>
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_assign_model(ekf_handle *h, const ekf_model_obs *o, int64_t m, ekf_model_assigned *out, ekf_model_match *match, int64_t *cand,
                         double *cand_d2, double *total) {
    printf("ABI ekf_assign_model m=%lld match=%d cand=%d cand_d2=%d total=%d\n", (long long)m, match != 0, cand != 0, cand_d2 != 0, total != 0);
    for (int64_t k = 0; k < m; ++k)
        printf("ABI   obs model=%d reserved=%d z=%g,%g R=%g,%g,%g,%g lm=%lld,%lld anchor=%g,%g gate=%g\n", (int)o[k].model, (int)o[k].reserved, o[k].z[0],
               o[k].z[1], o[k].R[0], o[k].R[1], o[k].R[2], o[k].R[3], (long long)o[k].lm[0], (long long)o[k].lm[1], o[k].anchor[0], o[k].anchor[1], o[k].gate);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    for (int64_t k = 0; k < m; ++k) {
        out[k].landmark = k == 0 ? 2 : -1; out[k].d2 = k == 0 ? 0.75 : INFINITY; out[k].ncand = k == 0 ? 2 : 0; out[k].reserved = 0;
        match[k].best = k == 0 ? 1 : -1; match[k].second = k == 0 ? 2 : -1;
        match[k].d2_best = k == 0 ? 0.5 : INFINITY; match[k].d2_second = k == 0 ? 0.75 : INFINITY;
        match[k].within_gate = k == 0 ? 2 : 0; match[k].irregular = 10 * k;
        for (int s = 0; cand && s < EKF_ASSIGN_CANDIDATES; ++s) {                      /* row-major m x 32 */
            cand[k * EKF_ASSIGN_CANDIDATES + s] = k == 0 && s < 2 ? 1 + s : -1;
            cand_d2[k * EKF_ASSIGN_CANDIDATES + s] = k == 0 && s < 2 ? 0.5 + 0.25 * s : INFINITY;
        }
    }
    *total = 0.75 + o[1].gate;
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *sx[3] = { mock_string("set_x"), h, mock_double(9, 1, (const double[]){ 0, 0, 0, 1, 2, 3, 4, 5, 6 }) };      /* three landmarks */
    if (call("set_x", 0, 3, sx)) return 1;
    /* a scan of two: range and bearing (7, 8), a range 7.5; z is m x 2 column-major, R 2 x 2 x m */
    const mxArray *model = mock_double(2, 1, (const double[]){ 1, 2 }), *z = mock_double(2, 2, (const double[]){ 7, 7.5, 8, 0 });
    const mxArray *R = mock_double(4, 2, (const double[]){ 4, 1, 1, 9, 0.5, 0, 0, 0 }), *gate = mock_double(2, 1, (const double[]){ 9.5, 4.0 });
    const mxArray *am[6] = { mock_string("assign_model"), h, model, z, R, gate };
    if (call("assign_model", 2, 6, am)) return 1;
    if (call("assign_model lists", 4, 6, am)) return 1;
    const mxArray *bad[6];
    for (int q = 0; q < 6; ++q) bad[q] = am[q];
    if (!call("assign_model", 1, 5, am)) return 1;
    bad[2] = mock_double(0, 0, 0);
    if (!call("assign_model none", 1, 6, bad)) return 1;
    bad[2] = mock_double(33, 1, 0);
    if (!call("assign_model many", 1, 6, bad)) return 1;
    bad[2] = model; bad[3] = mock_double(2, 1, (const double[]){ 7, 8 });
    if (!call("assign_model badz", 1, 6, bad)) return 1;
    bad[3] = z; bad[4] = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    if (!call("assign_model badr", 1, 6, bad)) return 1;
    bad[4] = R; bad[5] = D1(9.5);
    if (!call("assign_model badgate", 1, 6, bad)) return 1;
    bad[5] = gate; bad[1] = D1(1);
    if (!call("assign_model noh", 1, 6, bad)) return 1;
    arm_failure();
    if (!call("assign_model", 1, 6, am)) return 1;
''', SHOWN4)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *am[6] = { mock_string("assign_model"), h, D1(1), mock_double(1, 2, 0), mock_double(2, 2, 0), D1(1) };
    if (!call("assign_model", 1, 6, am)) return 1;
''')


def test_mex_gateway_marshals_a_scan_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # every entry searches: lm = {-1, -1}, the anchor zero; R column-major as MATLAB holds it; the lists only where a third output is asked for
    i = t.index("ABI ekf_assign_model m=2 match=1 cand=0 cand_d2=0 total=1")
    assert t[i + 1] == "ABI   obs model=1 reserved=0 z=7,8 R=4,1,1,9 lm=-1,-1 anchor=0,0 gate=9.5"
    assert t[i + 2] == "ABI   obs model=2 reserved=0 z=7.5,0 R=0.5,0,0,0 lm=-1,-1 anchor=0,0 gate=4"
    # landmarks 1-based with 0 = left out / none; one row per observation: landmark d2 ncand best second d2_best d2_second within_gate irregular
    row = "out0=2x9[3,0,0.75,inf,2,0,2,0,3,0,0.5,inf,0.75,inf,2,0,0,10] out1=1x1[4.75]"
    assert t[i + 3] == "MEX assign_model nrhs=6 -> ok " + row
    i = t.index("ABI ekf_assign_model m=2 match=1 cand=1 cand_d2=1 total=1")
    shown = t[i + 3]
    assert shown.startswith("MEX assign_model lists nrhs=6 -> ok " + row + " out2=2x32[2,0,3,0,0,0,") and " out3=2x32[0.5,inf,0.75,inf,inf,inf," in shown
    assert any(ln.startswith("MEX assign_model nrhs=5 -> ERROR ekfslam:usage") and "needs 6 arguments" in ln for ln in t)
    for which, what in (("none", "between 1 and 32 observations"), ("many", "between 1 and 32 observations"), ("badz", "z needs m x 2 elements"),
                        ("badr", "R needs 2 x 2 x m elements"), ("badgate", "gate needs m elements")):
        assert any(ln.startswith("MEX assign_model %s nrhs=6 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX assign_model noh nrhs=6 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_assign_model") for ln in t) == 3             # the two good calls and the injected failure
    assert "MEX assign_model nrhs=6 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX assign_model ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_assign_model" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+\[res,\s*total,\s*cand,\s*candD2\]\s*=\s*assignModel\(h,\s*model,\s*z,\s*R,\s*gate\)(.*?)\n        end\b", text, re.S)
    assert m and m.group(1).count("h.gateway('assign_model', model, z, R, gate)") == 2
    m = re.search(r"function\s+out\s*=\s*measureModelAssigned\(h,\s*model,\s*z,\s*R,\s*gateMatch,\s*gateNew,\s*signature\)(.*?)\n        end\n        function", text, re.S)
    body = m.group(1)
    assert "h.assignModel(model, z, R, gateMatch)" in body and "h.addLandmarksModel(" in body
    assert re.search(r"h\.observeModel\(model\(k\),\s*z\(k, :\),\s*R\(:, :, k\),\s*res\(k, 1\),\s*\[\],\s*gateMatch,", body)
    assert body.index("h.observeModel(") < body.index("h.addLandmarksModel(")               # the matched ones first, then ONE append
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "assign_model")' in src and "#pragma weak ekf_assign_model" in src
