"""CPU: the MEX gateway's `predict_model` command under the MEX mock with a recording stand-in for ekf_predict_model, the gateway linked
against a stand-in that lacks the symbol, and the MATLAB methods that forward to the command."""
import os
import re

from mex_harness import OPEN_SILENT, ROOT, driver, driver_without, transcript_of

_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_predict_model(ekf_handle *h, const ekf_motion *o, int64_t m) {
    printf("ABI ekf_predict_model m=%lld\n", (long long)m);
    for (int64_t b = 0; b < m; ++b) {
        printf("ABI   step model=%d reserved=%d u=%g,%g,%g M=", (int)o[b].model, (int)o[b].reserved, o[b].u[0], o[b].u[1], o[b].u[2]);
        for (int q = 0; q < 9; ++q) printf(q ? ",%g" : "%g", o[b].M[q]);
        printf("\n");
    }
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    /* one step: turn 30, drive 5 */
    const mxArray *u1 = mock_double(1, 3, (const double[]){ 5, 30, 0 }), *M1 = mock_double(3, 3, (const double[]){ 4, 1, 0, 1, 9, 0, 0, 0, 0 });
    const mxArray *one[5] = { mock_string("predict_model"), h, D1(1), u1, M1 };
    if (call("predict_model", 0, 5, one)) return 1;
    /* a chain of two: u is 2 x 3 column-major, M 3 x 3 x 2 */
    const mxArray *model2 = mock_double(2, 1, (const double[]){ 2, 3 }), *u2 = mock_double(2, 3, (const double[]){ 1.5, 0.25, 10, -0.5, 0, 45 });
    const double m2[18] = { 4, 1, 0, 1, 9, 0, 0, 0, 0, 1, 0.1, 0.2, 0.1, 2, 0.3, 0.2, 0.3, 3 };
    const mxArray *M2 = mock_double(9, 2, m2);
    const mxArray *two[5] = { mock_string("predict_model"), h, model2, u2, M2 };
    if (call("predict_model two", 0, 5, two)) return 1;
    const mxArray *bad[5];
    for (int q = 0; q < 5; ++q) bad[q] = two[q];
    if (!call("predict_model", 0, 4, two)) return 1;
    bad[2] = mock_double(0, 0, 0);
    if (!call("predict_model none", 0, 5, bad)) return 1;
    double many[33] = { 0 };
    bad[2] = mock_double(33, 1, many);
    if (!call("predict_model many", 0, 5, bad)) return 1;
    bad[2] = model2; bad[3] = u1;
    if (!call("predict_model badu", 0, 5, bad)) return 1;
    bad[3] = mock_double(2, 2, (const double[]){ 1, 2, 3, 4 });
    if (!call("predict_model badu2", 0, 5, bad)) return 1;
    bad[3] = u2; bad[4] = M1;
    if (!call("predict_model badm", 0, 5, bad)) return 1;
    bad[4] = M2; bad[1] = D1(1);
    if (!call("predict_model noh", 0, 5, bad)) return 1;
    arm_failure();
    if (!call("predict_model", 0, 5, one)) return 1;
''')

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *pm[5] = { mock_string("predict_model"), h, D1(1), mock_double(1, 3, (const double[]){ 5, 30, 0 }), mock_double(3, 3, (const double[]){ 4, 1, 0, 1, 9, 0, 0, 0, 0 }) };
    if (!call("predict_model", 0, 5, pm)) return 1;
''', OPEN_SILENT)


def test_mex_gateway_marshals_a_chain_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # u row by row out of the column-major m x 3; M column-major as MATLAB holds it, page by page
    i = t.index("ABI ekf_predict_model m=1")
    assert t[i + 1] == "ABI   step model=1 reserved=0 u=5,30,0 M=4,1,0,1,9,0,0,0,0"
    assert t[i + 2] == "MEX predict_model nrhs=5 -> ok"
    i = t.index("ABI ekf_predict_model m=2")
    assert t[i + 1] == "ABI   step model=2 reserved=0 u=1.5,10,0 M=4,1,0,1,9,0,0,0,0"
    assert t[i + 2] == "ABI   step model=3 reserved=0 u=0.25,-0.5,45 M=1,0.1,0.2,0.1,2,0.3,0.2,0.3,3"
    assert t[i + 3] == "MEX predict_model two nrhs=5 -> ok"
    assert any(ln.startswith("MEX predict_model nrhs=4 -> ERROR ekfslam:usage") and "needs 5 arguments" in ln for ln in t)
    for which, what in (("none", "between 1 and 32 steps"), ("many", "between 1 and 32 steps"), ("badu", "u needs m x 3 elements"),
                        ("badu2", "u needs m x 3 elements"), ("badm", "M needs 3 x 3 x m elements")):
        assert any(ln.startswith("MEX predict_model %s nrhs=5 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX predict_model noh nrhs=5 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_predict_model") for ln in t) == 3           # the two good calls and the injected failure
    assert "MEX predict_model nrhs=5 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX predict_model ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_predict_model" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+predictModel\(h,\s*model,\s*u,\s*M\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('predict_model', model, u, M3)" in m.group(1) and "Not a method of" in m.group(1)
    for name, inner in (("predictTurnDrive", r"h\.predictModel\(ones\("), ("predictArc", r"h\.predictModel\(2 \* ones\("),
                        ("predictPoseDelta", r"h\.predictModel\(3 \* ones\(")):
        m = re.search(r"function\s+%s\((.*?)\n        end\b" % name, text, re.S)
        assert m and re.search(inner, m.group(1)), name
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "predict_model")' in src and "#pragma weak ekf_predict_model" in src
