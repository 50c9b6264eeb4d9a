"""CPU: the MEX gateway's `observe_model` command under the MEX mock with a recording stand-in for ekf_observe_model, the gateway
linked against a stand-in that lacks the symbol, and the MATLAB methods that forward to the command."""
import os
import re

from mex_harness import PRELUDE_SHOWN, ROOT, driver, driver_without, transcript_of

_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_observe_model(ekf_handle *h, const ekf_model_obs *o, ekf_linear_result *res) {
    printf("ABI ekf_observe_model model=%d reserved=%d z=%g,%g R=%g,%g,%g,%g lm=%lld,%lld anchor=%g,%g gate=%g wait=%d\n", (int)o->model, (int)o->reserved,
           o->z[0], o->z[1], o->R[0], o->R[1], o->R[2], o->R[3], (long long)o->lm[0], (long long)o->lm[1], o->anchor[0], o->anchor[1], o->gate, res != 0);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    if (res) { res->nu[0] = 0.5; res->nu[1] = -0.25; res->S[0] = 1; res->S[1] = 2; res->S[2] = 3; res->S[3] = 4; res->d2 = 1.5; res->outcome = EKF_LINEAR_GATED; }
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *z = mock_double(2, 1, (const double[]){ 7, 8 }), *R = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    const mxArray *lm1 = D1(5), *lm2 = mock_double(2, 1, (const double[]){ 5, 3 }), *none = mock_double(0, 0, 0);
    const mxArray *anchor = mock_double(2, 1, (const double[]){ 10, -4 });
    /* range and bearing to landmark 5 (1-based), no wait */
    const mxArray *rb[9] = { mock_string("observe_model"), h, D1(1), z, R, lm1, none, D1(9.5), D1(0) };
    if (call("observe_model", 1, 9, rb)) return 1;
    /* the range to an anchor, the result waited for */
    const mxArray *an[9] = { mock_string("observe_model"), h, D1(2), mock_double(2, 1, (const double[]){ 7.5, 0 }), mock_double(2, 2, (const double[]){ 0.5, 0, 0, 0 }),
                             none, anchor, D1(1.0 / 0.0), D1(1) };
    if (call("observe_model anchor", 1, 9, an)) return 1;
    /* the distance between landmarks 5 and 3 */
    const mxArray *lr[9] = { mock_string("observe_model"), h, D1(5), mock_double(2, 1, (const double[]){ 2.5, 0 }), mock_double(2, 2, (const double[]){ 0.1, 0, 0, 0 }),
                             lm2, none, D1(4), D1(0) };
    if (call("observe_model pair", 1, 9, lr)) return 1;
    const mxArray *bad[9];
    for (int q = 0; q < 9; ++q) bad[q] = rb[q];
    if (!call("observe_model", 1, 8, rb)) return 1;
    bad[5] = mock_double(3, 1, (const double[]){ 1, 2, 3 });
    if (!call("observe_model three", 1, 9, bad)) return 1;
    bad[5] = lm1; bad[6] = anchor;
    if (!call("observe_model both", 1, 9, bad)) return 1;
    bad[5] = none; bad[6] = none;
    if (!call("observe_model neither", 1, 9, bad)) return 1;
    bad[6] = mock_double(3, 1, (const double[]){ 1, 2, 3 });
    if (!call("observe_model anchor3", 1, 9, bad)) return 1;
    bad[5] = D1(1.5); bad[6] = none;
    if (!call("observe_model frac", 1, 9, bad)) return 1;
    bad[5] = lm1; bad[4] = mock_double(2, 1, (const double[]){ 1, 2 });
    if (!call("observe_model badr", 1, 9, bad)) return 1;
    bad[4] = R; bad[3] = D1(1);
    if (!call("observe_model badz", 1, 9, bad)) return 1;
    bad[3] = z; bad[1] = D1(1);
    if (!call("observe_model noh", 1, 9, bad)) return 1;
    arm_failure();
    if (!call("observe_model", 1, 9, rb)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *ob[9] = { mock_string("observe_model"), h, D1(2), mock_double(2, 1, 0), mock_double(2, 2, 0), D1(1), mock_double(0, 0, 0), D1(1), D1(0) };
    if (!call("observe_model", 1, 9, ob)) return 1;
''')


def test_mex_gateway_marshals_a_model_observation_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # MATLAB's lm = 5 arrives 0-based once, R column-major as MATLAB holds it; no result asked for: an empty output
    i = t.index("ABI ekf_observe_model model=1 reserved=0 z=7,8 R=4,1,1,9 lm=4,-1 anchor=0,0 gate=9.5 wait=0")
    assert t[i + 1] == "MEX observe_model nrhs=9 -> ok out0=0x0[]"
    i = t.index("ABI ekf_observe_model model=2 reserved=0 z=7.5,0 R=0.5,0,0,0 lm=-1,-1 anchor=10,-4 gate=inf wait=1")
    assert t[i + 1] == "MEX observe_model anchor nrhs=9 -> ok out0=1x8[0.5,-0.25,1,2,3,4,1.5,2]"
    i = t.index("ABI ekf_observe_model model=5 reserved=0 z=2.5,0 R=0.1,0,0,0 lm=4,2 anchor=0,0 gate=4 wait=0")
    assert t[i + 1] == "MEX observe_model pair nrhs=9 -> ok out0=0x0[]"
    assert any(ln.startswith("MEX observe_model nrhs=8 -> ERROR ekfslam:usage") and "needs 9 arguments" in ln for ln in t)
    for which, what in (("three", "at most two landmarks"), ("both", "a landmark (anchor empty) or an anchor"), ("neither", "a landmark (anchor empty) or an anchor"),
                        ("anchor3", "an anchor of 2 elements"), ("frac", "whole numbers"), ("badr", "R needs 2 x 2 elements"), ("badz", "z needs 2 elements")):
        assert any(ln.startswith("MEX observe_model %s nrhs=9 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX observe_model noh nrhs=9 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_observe_model") for ln in t) == 4          # the three good calls and the injected failure
    assert "MEX observe_model nrhs=9 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX observe_model ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_observe_model" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+res\s*=\s*observeModel\(h,\s*model,\s*z,\s*R,\s*lm,\s*anchor,\s*gate,\s*wait\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('observe_model'," in m.group(1)
    for name, inner in (("observeRangeBearing", r"h\.observeModel\(1,\s*z,\s*R,\s*i,\s*\[\],"), ("observeRange", r"h\.observeModel\(2,\s*\[r 0\],\s*\[variance 0; 0 0\],\s*i,\s*\[\],"),
                        ("observeBearing", r"h\.observeModel\(3,\s*\[deg 0\],\s*\[variance 0; 0 0\],\s*i,\s*\[\],"), ("observeRelativeXY", r"h\.observeModel\(4,\s*z,\s*R,\s*i,\s*\[\],"),
                        ("observeLandmarkRange", r"h\.observeModel\(5,\s*\[dist 0\],\s*\[variance 0; 0 0\],\s*\[i j\],\s*\[\],"),
                        ("observeAnchorRange", r"h\.observeModel\(2,\s*\[r 0\],\s*\[variance 0; 0 0\],\s*\[\],\s*pos,"),
                        ("observeAnchorBearing", r"h\.observeModel\(3,\s*\[deg 0\],\s*\[variance 0; 0 0\],\s*\[\],\s*pos,")):
        m = re.search(r"function\s+res\s*=\s*%s\((.*?)\n        end\b" % name, text, re.S)
        assert m and re.search(inner, m.group(1)), name
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "observe_model")' in src and "#pragma weak ekf_observe_model" in src
