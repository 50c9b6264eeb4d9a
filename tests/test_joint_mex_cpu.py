"""CPU: the MEX gateway's `joint_innovation` command under the MEX mock with a recording stand-in for ekf_joint_innovation, the gateway
linked against a stand-in that lacks the symbol, and the MATLAB method that forwards to the command."""
import os
import re

from mex_harness import PRELUDE_SHOWN, ROOT, driver, driver_without, transcript_of

_STUB = r'''
#include <math.h>
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_joint_innovation(ekf_handle *h, const ekf_model_obs *o, int64_t m, const int64_t *hyp, int64_t nh, ekf_joint_result *out,
                             double *d2_prefix, double *nu, double *S) {
    printf("ABI ekf_joint_innovation m=%lld nh=%lld prefix=%d nu=%d S=%d\n", (long long)m, (long long)nh, d2_prefix != 0, nu != 0, S != 0);
    for (int64_t k = 0; k < m; ++k)
        printf("ABI   obs model=%d reserved=%d z=%g,%g R=%g,%g,%g,%g lm=%lld,%lld anchor=%g,%g gate=%g\n", (int)o[k].model, (int)o[k].reserved, o[k].z[0],
               o[k].z[1], o[k].R[0], o[k].R[1], o[k].R[2], o[k].R[3], (long long)o[k].lm[0], (long long)o[k].lm[1], o[k].anchor[0], o[k].anchor[1], o[k].gate);
    for (int64_t i = 0; i < nh; ++i) {
        printf("ABI   hyp");
        for (int64_t k = 0; k < m; ++k) printf(" %lld", (long long)hyp[i * m + k]);
        printf("\n");
    }
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    for (int64_t i = 0; i < nh; ++i) {
        out[i].d2 = i == 0 ? 0.25 : NAN; out[i].dof = 4 - (int32_t)i; out[i].pairings = 2 - (int32_t)i;
        out[i].outcome = i == 0 ? EKF_LINEAR_APPLIED : EKF_LINEAR_IRREGULAR; out[i].first_irregular = i == 0 ? -1 : 1;
        if (d2_prefix) for (int64_t k = 0; k < m; ++k) d2_prefix[i * m + k] = 10.0 * (double)i + (double)k;      /* row-major nh x m */
    }
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    /* a scan of two (range and bearing (7, 8), a range 7.5) and three hypotheses, nh x m column-major: [2 3; 0 1; 3 0] */
    const mxArray *model = mock_double(2, 1, (const double[]){ 1, 2 }), *z = mock_double(2, 2, (const double[]){ 7, 7.5, 8, 0 });
    const mxArray *R = mock_double(4, 2, (const double[]){ 4, 1, 1, 9, 0.5, 0, 0, 0 }), *hyp = mock_double(3, 2, (const double[]){ 2, 0, 3, 3, 1, 0 });
    const mxArray *ji[6] = { mock_string("joint_innovation"), h, model, z, R, hyp };
    if (call("joint_innovation", 1, 6, ji)) return 1;
    if (call("joint_innovation prefix", 2, 6, ji)) return 1;
    const mxArray *bad[6];
    for (int q = 0; q < 6; ++q) bad[q] = ji[q];
    if (!call("joint_innovation", 1, 5, ji)) return 1;
    bad[2] = mock_double(0, 0, 0);
    if (!call("joint_innovation none", 1, 6, bad)) return 1;
    bad[2] = mock_double(33, 1, 0);
    if (!call("joint_innovation many", 1, 6, bad)) return 1;
    bad[2] = model; bad[3] = mock_double(2, 1, (const double[]){ 7, 8 });
    if (!call("joint_innovation badz", 1, 6, bad)) return 1;
    bad[3] = z; bad[4] = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    if (!call("joint_innovation badr", 1, 6, bad)) return 1;
    bad[4] = R; bad[5] = mock_double(3, 1, (const double[]){ 2, 0, 3 });
    if (!call("joint_innovation badhyp", 1, 6, bad)) return 1;
    bad[5] = mock_double(257, 2, 0);
    if (!call("joint_innovation manyhyp", 1, 6, bad)) return 1;
    bad[5] = mock_double(1, 2, (const double[]){ 1.5, 2 });
    if (!call("joint_innovation fraction", 1, 6, bad)) return 1;
    bad[5] = mock_double(1, 2, (const double[]){ -1, 2 });
    if (!call("joint_innovation negative", 1, 6, bad)) return 1;
    bad[5] = hyp; bad[1] = D1(1);
    if (!call("joint_innovation noh", 1, 6, bad)) return 1;
    arm_failure();
    if (!call("joint_innovation", 1, 6, ji)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *ji[6] = { mock_string("joint_innovation"), h, D1(1), mock_double(1, 2, 0), mock_double(2, 2, 0), D1(1) };
    if (!call("joint_innovation", 1, 6, ji)) return 1;
''')


def test_mex_gateway_marshals_the_hypotheses_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # every entry searches: lm = {-1, -1}, the anchor zero, the gate open; the hypotheses row-major and 0-based, 0 (left out) -> -1
    i = t.index("ABI ekf_joint_innovation m=2 nh=3 prefix=0 nu=0 S=0")
    assert t[i + 1] == "ABI   obs model=1 reserved=0 z=7,8 R=4,1,1,9 lm=-1,-1 anchor=0,0 gate=inf"
    assert t[i + 2] == "ABI   obs model=2 reserved=0 z=7.5,0 R=0.5,0,0,0 lm=-1,-1 anchor=0,0 gate=inf"
    assert t[i + 3:i + 6] == ["ABI   hyp 1 2", "ABI   hyp -1 0", "ABI   hyp 2 -1"]
    # one row per hypothesis: d2 dof pairings outcome firstIrregular (1-based, 0 = none), column-major here
    shown = "out0=3x5[0.25,nan,nan,4,3,2,2,1,0,1,0,0,0,2,2]"
    assert t[i + 6].replace("-nan", "nan") == "MEX joint_innovation nrhs=6 -> ok " + shown
    i = t.index("ABI ekf_joint_innovation m=2 nh=3 prefix=1 nu=0 S=0")
    assert t[i + 6].replace("-nan", "nan") == "MEX joint_innovation prefix nrhs=6 -> ok " + shown + " out1=3x2[0,10,20,1,11,21]"      # nh x m
    assert any(ln.startswith("MEX joint_innovation nrhs=5 -> ERROR ekfslam:usage") and "needs 6 arguments" in ln for ln in t)
    for which, what in (("none", "between 1 and 32 observations"), ("many", "between 1 and 32 observations"), ("badz", "z needs m x 2 elements"),
                        ("badr", "R needs 2 x 2 x m elements"), ("badhyp", "hyp needs nh x m elements"), ("manyhyp", "between 1 and 256 hypotheses"),
                        ("fraction", "landmark numbers (1-based)"), ("negative", "landmark numbers (1-based)")):
        assert any(ln.startswith("MEX joint_innovation %s nrhs=6 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX joint_innovation noh nrhs=6 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_joint_innovation") for ln in t) == 3           # the two good calls and the injected failure
    assert "MEX joint_innovation nrhs=6 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX joint_innovation ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_joint_innovation" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_forwards_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+\[res,\s*prefix\]\s*=\s*jointInnovation\(h,\s*model,\s*z,\s*R,\s*hyp\)(.*?)\n        end\b", text, re.S)
    assert m and m.group(1).count("h.gateway('joint_innovation', model, z, R, hyp)") == 2
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "joint_innovation")' in src and "#pragma weak ekf_joint_innovation" in src
