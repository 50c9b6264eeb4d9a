"""CPU: which kernel instance a pass over P runs (ekf_slam_amd/csrc/launch/pass_select.h, a header without HIP), compiled for the host
behind tests/support/pass_select_harness.cpp: every combination of storage, tile edge, 1-64 pairs, pass arithmetic, XCD list, strip list
with planes, next row -- against the full-batch rule of tests/random_plans.py and a restatement of the table of DESIGN.md section 3."""
import os
import re
import subprocess

import pytest

from random_plans import ROWS, expected_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("family", "slab", "chunk", "cols", "early", "xcd", "rowpanel")
WIDE = {(8, 64), (8, 128), (4, 128), (4, 256)}                     # a tile row of 32 or 64 lanes of 16 bytes: k_downdate_w
MATRIX_FAMILIES = {1, 2, 3, 4}                                     # ekf_pass::kSplit3 .. kMfma64
# slab with no override: (one pair, several pairs); and what EKF_DOWNDATE_SLAB / _SLAB_BATCH may name per storage and tile edge
SLAB = {(8, 16): (16, 16), (8, 32): (16, 16), (8, 64): (8, 64), (8, 128): (4, 32),
        (4, 16): (16, 16), (4, 32): (32, 32), (4, 64): (64, 64), (4, 128): (8, 64), (4, 256): (4, 32)}
OVERRIDES = {(8, 32): {32}, (8, 64): {64, 32, 16, 8}, (8, 128): {32, 16, 8, 4}, (4, 256): {32, 16, 8, 4}}
STORAGE = {"f64": (8, 0), "f32": (4, 0), "f32_mixed": (4, 1), "f32_split": (4, 2)}      # element bytes, cfg.pass_arith


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pass_select") / "harness")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ekf_slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "support", "pass_select_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(slab_override=0):
        out = subprocess.run([exe, str(slab_override)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        table = {}
        for line in out.stdout.splitlines():
            key, val = line.split(" | ")
            v = val.split(" ", len(FIELDS))
            table[tuple(int(k) for k in key.split())] = dict(zip(FIELDS, (int(x) for x in v[:-1])), name=v[-1])
        return table
    return run


def table_name(elt, T, np_, arith, xcd, strip, nxt):
    """The contract: the parent's launch_downdate_t / launch_downdate_ts / launch_flush_mfma at product defaults, row by row."""
    ts = "double" if elt == 8 else "float"
    if (elt, T) == (4, 256) and xcd:
        if arith == 2 and 28 <= np_ <= 64 and strip:
            return "k_flush_split3<2>"
        if arith == 1 and 57 <= np_ <= 64 and strip:
            return "k_flush_strip32<8>"
        if arith >= 1 and np_ > 2:
            return "k_flush_mfma32<256,4,2,3>" if np_ <= 4 else "k_flush_mfma32<256,4,2,3,early>"
        return "k_flush_mfma<float,256,4>" if np_ <= 30 else "k_flush_mfma<float,256,8>"
    if (elt, T) == (8, 128) and xcd and np_ >= 2:
        return "k_flush_mfma<double,128,4,64>" if np_ <= 12 else "k_flush_mfma<double,128,4>" if np_ <= 30 else "k_flush_mfma<double,128,8>"
    slab = SLAB[(elt, T)][np_ > 1]
    if (elt, T) not in WIDE:
        return "k_downdate<%s,%d,%d>" % (ts, T, slab)
    if np_ > 1 and xcd:
        return "k_downdate_w<%s,%d,%d,true>" % (ts, T, slab)
    if np_ == 1 and nxt:
        return "k_downdate_w<%s,%d,%d,false,+rowpanel>" % (ts, T, slab)
    return "k_downdate_w<%s,%d,%d,false>" % (ts, T, slab)


def _every_combination_is_printed_once(got):
    want = {(elt, T, np_, arith, xcd, strip, nxt)
            for elt, tiles in ((8, (16, 32, 64, 128)), (4, (16, 32, 64, 128, 256))) for T in tiles for np_ in range(1, 65)
            for arith in ((0, 1, 2) if (elt, T) == (4, 256) else (0,)) for xcd in (0, 1) for strip in (0, 1) for nxt in (0, 1)}
    assert set(got) == want and len(want) == 8 * 64 * (4 + 4 + 3)


def _full_batches_select_what_the_random_plans_expect(got):
    seen = set()
    for storage, tiles, batches in ROWS:
        elt, arith = STORAGE[storage]
        for T in tiles:
            for batch in batches:
                name = got[(elt, T, batch, arith, 1, 1, 0)]["name"]
                prefix = expected_kernel(storage, T, batch)
                assert name.startswith(prefix), (storage, T, batch, name, prefix)
                assert name in (prefix, prefix + ">"), (name, prefix)         # (a prefix only leaves the closing bracket open)
                seen.add(prefix)
    asserted = set(re.findall(r'"(k_[^"]+)"', open(os.path.join(ROOT, "tests", "test_random_plans_cpu.py")).read()))
    assert len(asserted) == 16 and seen == asserted, sorted(seen ^ asserted)


def _every_combination_equals_the_table(got):
    for key, inst in got.items():
        elt, T, np_, arith, xcd, strip, nxt = key
        assert inst["name"] == table_name(*key), (key, inst["name"])
        assert inst["slab"] == SLAB[(elt, T)][np_ > 1], key
        assert inst["rowpanel"] == int(inst["name"].endswith(",+rowpanel>")), key      # what launch_downdate reports as *extracted


def _slab_overrides(harness, base):
    # no tile edge accepts 5: the default stays
    assert harness(5) == base
    for slab in (4, 8, 16, 32, 64):
        got = harness(slab)
        for key, inst in got.items():
            elt, T = key[:2]
            was = base[key]
            if slab not in OVERRIDES.get((elt, T), ()):
                assert inst == was, (slab, key)
                continue
            # a supported override moves the slab and nothing else (the VALU kernels' names carry the slab)
            assert inst["slab"] == slab and all(inst[f] == was[f] for f in FIELDS if f != "slab"), (slab, key)
            if was["family"] in MATRIX_FAMILIES:
                assert inst["name"] == was["name"], (slab, key)
            else:
                assert inst["name"] == was["name"].replace(",%d%s" % (was["slab"], ",t" if was["xcd"] else ",f" if (elt, T) in WIDE else ">"),
                                                           ",%d%s" % (slab, ",t" if was["xcd"] else ",f" if (elt, T) in WIDE else ">"), 1), (slab, key)


def test_pass_selection(harness):
    got = harness()
    _every_combination_is_printed_once(got)
    _full_batches_select_what_the_random_plans_expect(got)
    _every_combination_equals_the_table(got)
    _slab_overrides(harness, got)
