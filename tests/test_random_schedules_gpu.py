"""GPU: seeded random schedules on every production pass kernel (tests/random_plans.py draws the plans; test_random_plans_cpu.py checks
them without a GPU).

Each seed runs three things side by side: the CONFIGURED engine (a plain handle, a ShardGroup of 2-4 shards, or a one-rank handle on the
library's own RCCL communicator), a TWIN (unsharded, synchronous; F64 tiles: batch 1; float tiles: the configured storage, tile and
batch) and the structured F64 oracle.  The configured engine is read only every `cadence`-th op, so that recorded predicts, passes in
flight and unverified device decisions live across ops; observations come from the oracle's x (host only).  Every op that flushes is
applied to the configured engine and the twin alike.  After every reload (a shrinking ekf_set_x, a low-rank load, a checkpoint loaded
into a handle that has grown since the save) the twin is replaced by a NEW handle given the same state: the configured handle, reused,
is compared with one that has no history.

Bars (max-norm, relative to the largest |x| / |P| entry of the whole state):
  F64 tiles, any schedule       configured == twin bit for bit; both within 1e-10 of the oracle
  float tiles, synchronous      configured == twin bit for bit (sharding moves no operation); both within 1e-6 of the oracle
  float tiles, asynchronous     configured within 2e-6 of the synchronous twin; both within 1e-6 of the oracle
Every seed also asserts that the pass kernel its full batch selects ran (ekf_downdate_kernel_name, sampled after every op)."""
import ctypes
import os
import time

import numpy as np
import pytest

from random_plans import NSEEDS, describe, plan

pytestmark = pytest.mark.gpu
ORACLE_F64, ORACLE_FLOAT, ASYNC_FLOAT = 1e-10, 1e-6, 2e-6


def rel(a, b, scale):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(scale, 1e-300))


class _Table:
    """Landmark.m-shaped source handing the oracle the same observed rows / landmark table the GPU call gets."""
    def __init__(self, rows, index, loc):
        class _E:
            def __init__(self, i, l): self.index, self.loc = i, np.asarray(l, dtype=float)
        class _O: pass
        self.rows = np.asarray(rows, dtype=float).reshape(-1, 3)
        self.landmarkObj = _O()
        self.landmarkObj.landmark = [_E(i, l) for i, l in zip(index, loc)]

    def getLandmark(self, laser, x):
        return self.rows


def _rccl_loads():
    """Whether librccl loads under the names the library tries (csrc/host/exchange.h: rccl_load)."""
    for name in ("librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"):
        try:
            ctypes.CDLL(name, mode=ctypes.RTLD_GLOBAL)
            return True
        except OSError:
            pass
    return False


def _merge(parts):
    """A shard's view holds NaN where another shard owns the entry."""
    out = parts[0].copy()
    for q in parts[1:]:
        hole = np.isnan(out)
        out[hole] = q[hole]
    return out


class Configured:
    """The engine under test behind one surface: a plain Engine, a ShardGroup (transports (c)/(d)) or a one-rank communicator Engine."""

    def __init__(self, cfg, kw, tmp):
        from ekf_slam_amd import Engine, _lib as L
        from ekf_slam_amd.sharding import ShardGroup
        self.cfg, self.tmp = cfg, tmp
        ekw = dict(kw, batch=cfg["batch"], async_flush=cfg["async_flush"], device_assoc=cfg["device_assoc"])
        sh = cfg["shards"]
        self.group = None
        if sh == "comm":
            if not _rccl_loads():
                pytest.skip("librccl not loadable")
            raw = ctypes.create_string_buffer(L.EKF_COMM_ID_BYTES)
            assert L.lib().ekf_comm_unique_id(raw) == 0       # librccl loads: the library's id path must work
            e = Engine(force_sharded=1, **ekw)
            e.comm_init(raw.raw)
            self.engines = [e]
        elif sh > 1:
            self.group = ShardGroup(sh, **ekw)
            self.engines = self.group.shards
        else:
            self.engines = [Engine(**ekw)]
        self.front = self.group if self.group is not None else self.engines[0]

    def close(self):
        for e in self.engines:
            e.close()

    @property
    def N(self):
        return self.engines[0].N

    def kernels(self):
        """(name, pairs) of every shard's last pass launch"""
        return {e.downdate_kernel_name() for e in self.engines}

    def set_params(self, **kw):
        for e in self.engines:
            e.set_params(**kw)

    def get_x(self):
        return self.front.get_x()

    def get_P(self):
        return self.front.get_P()

    def diag(self):
        return _merge([e.get_P_diag_blocks() for e in self.engines])

    def pblock(self, r0, c0, nr, nc):
        return _merge([e.get_P_block(r0, c0, nr, nc) for e in self.engines])

    def correct(self, z, R, k, local=False):
        if local and self.group is not None:
            self.group.correct_local(z, R, k)
        else:
            self.front.correct(z, R, k)

    def measure(self, rows, u, idx, loc):
        self.front.measure(rows, u, idx, loc)

    def shrink(self, x):
        for e in self.engines:
            e._check(e.lib.ekf_set_x(e.h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x.size))

    def save(self, tag):
        for r, e in enumerate(self.engines):
            e.checkpoint_save(os.path.join(self.tmp, "cfg_%d_r%d.ckpt" % (tag, r)))

    def load(self, tag):
        for r, e in enumerate(self.engines):
            e.checkpoint_load(os.path.join(self.tmp, "cfg_%d_r%d.ckpt" % (tag, r)))

    def hint(self, k):
        for e in self.engines:
            e.hint_next(k)

    def prefetch(self, ks):
        self.front.prefetch_rows(ks)

    def prefetch_next_block(self, ks, corr):
        """The announcement and the corrections that complete the batch; on a group every shard on its own thread with the exchange hook
        (the batch's pass exchanges the announced row-panels inside the library)."""
        if self.group is None:
            self.engines[0].prefetch_next(ks)
            for z, R, k in corr:
                self.engines[0].correct(z, R, k)
            return

        def fn(e):
            e.prefetch_next(ks)
            for z, R, k in corr:
                e.correct(z, R, k)
        self.group.run_threaded(fn)


def _lowrank_data(N, seed):
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0, 90)], rng.uniform(-15, 15, size=2 * N)])
    return x, np.arange(1, N + 1.0), rng.uniform(0.01, 0.1, size=n), rng.normal(0, 0.05, size=(n, 5))


def _initial(N, seed):
    x, s, d, U = _lowrank_data(N, seed)
    return x, np.diag(d) + U @ U.T, s


def run_seed(seed, tmp):
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    cfg, ops = plan(seed)
    what = describe(cfg)
    st, floaty = cfg["storage"], cfg["storage"] != "f64"
    exact = not (floaty and cfg["async_flush"])
    bar = ORACLE_FLOAT if floaty else ORACLE_F64
    cap = cfg["cap"]
    kw = dict(mode="uc", capacity=cap, tile=cfg["tile"], storage=st)
    twin_kw = dict(kw, batch=cfg["batch"] if floaty else 1, device_assoc=0)
    params = dict(w_pos=cfg["w_pos"], s_cost=50.0, s_thresh=1e9)
    strict = dict(w_pos=0.0, s_cost=1e-3, s_thresh=1.0)   # measure(): a signature must match, the far row becomes a new landmark

    conf = Configured(cfg, kw, tmp)
    twin = Engine(**twin_kw)
    ref = StructuredEKF(cap, "uc")
    x0, P0, s0 = _initial(cfg["N0"], 5000 + seed)
    conf.front.set_state(x0, P0, s0); twin.set_state(x0, P0, s0); ref.set_state(x0, P0, s0)

    def set_params(p):
        conf.set_params(**p); twin.set_params(**p)
        ref.w_pos, ref.s_cost, ref.s_thresh = p["w_pos"], p["s_cost"], p["s_thresh"]
    set_params(params)

    def fresh_twin():
        t = Engine(**twin_kw)
        t.set_params(**params)
        return t

    worst = {"x": 0.0, "P": 0.0, "cost": 0.0, "twin": 0.0}
    kernels = set()
    snaps = {}
    since_read = []
    u = [0.1, 3.0]

    def obs(k, nz):
        xr = ref.x
        dx, dy = xr[3 + 2 * k] - xr[0], xr[4 + 2 * k] - xr[1]
        return [float(np.hypot(dx, dy) + .05 * nz[0]), float((np.degrees(np.arctan2(dy, dx)) - xr[2] + nz[1]) % 360.0)]

    def Rz(z):
        return np.array([[z[0] * .01, 0.001], [0.001, max(z[1], 1.0) * 5.0]])

    def agree(a, b, name, scale):
        """configured vs twin"""
        if exact:
            np.testing.assert_array_equal(a, b, err_msg=name)
        else:
            e = rel(a, b, scale)
            worst["twin"] = max(worst["twin"], e)
            assert e <= ASYNC_FLOAT, "%s: configured vs twin %.3g > %.0e" % (name, e, ASYNC_FLOAT)

    def to_oracle(a, b, scale, key, name):
        e = rel(a, b, scale)
        worst[key] = max(worst[key], e)
        assert e <= bar, "%s: %.3g against the oracle > %.0e" % (name, e, bar)

    def diag_of(P):
        """P(1:2,1:2) and every landmark's 2x2 diagonal block, as ekf_get_P_diag_blocks returns them"""
        N = (P.shape[0] - 3) // 2
        return np.stack([P[0:2, 0:2]] + [P[3 + 2 * q:5 + 2 * q, 3 + 2 * q:5 + 2 * q] for q in range(N)])

    def read(full=False):
        xc, xt, xr = conf.get_x(), twin.get_x(), ref.x
        Pr = ref.P
        sx, sP = np.abs(xr).max(), np.abs(Pr).max()
        assert conf.N == twin.N == ref.N
        agree(xc, xt, "x", sx)
        to_oracle(xc, xr, sx, "x", "x (configured)")
        to_oracle(xt, xr, sx, "x", "x (twin)")
        dc, dt, dr = conf.diag(), twin.get_P_diag_blocks(), diag_of(Pr)
        agree(dc, dt, "diagonal blocks", sP)
        to_oracle(dc, dr, sP, "P", "diagonal blocks (configured)")
        to_oracle(dt, dr, sP, "P", "diagonal blocks (twin)")
        if full:
            Pc, Pt = conf.get_P(), twin.get_P()
            agree(Pc, Pt, "P", sP)
            to_oracle(Pc, Pr, sP, "P", "P (configured)")
            to_oracle(Pt, Pr, sP, "P", "P (twin)")

    t0 = time.time()
    i = -1
    try:
        for i, o in enumerate(ops):
            since_read.append((i, o["op"]))
            kind = o["op"]
            N = ref.N
            if kind == "predict":
                u = o["u"]
                conf.front.predict(u); twin.predict(u); ref.predict(u)
            elif kind == "correct":
                z = obs(o["k"], o["nz"]); R = Rz(z)
                conf.correct(z, R, o["k"], o["local"]); twin.correct(z, R, o["k"]); ref.correct(z, R, o["k"] + 1)
            elif kind == "append":
                R = np.diag([0.2, 40.0])
                for e in (conf.front, twin, ref):
                    e.append(u, R, o["pos"], float(N + 1))
            elif kind == "associate":
                z = obs(o["k"], o["nz"]) + [float(o["sig"])]
                R = np.diag([z[0] * .1, max(z[1], 1.0) * 5.0])
                c = o["costs"]
                a, b, r = conf.front.associate(z, R, want_costs=c), twin.associate(z, R, want_costs=c), ref.associate(z, R, want_costs=c)
                assert a[:2] == b[:2] == (r[0], r[1] - 1), "association %s / %s / oracle %s" % (a[:2], b[:2], r[:2])
                if c:
                    for q in (2, 3):
                        sc = max(np.abs(r[q]).max(), 1e-300)
                        agree(a[q], b[q], "association costs", sc)
                        to_oracle(a[q], r[q], sc, "cost", "association costs (configured)")
                        to_oracle(b[q], r[q], sc, "cost", "association costs (twin)")
            elif kind == "measure":
                rows = [obs(k, nz) + [float(k + 1)] for k, nz in zip(o["ks"], o["nz"])]
                rows.append([4.0, 77.0, 5000.0 + i])
                idx, loc = np.array([N + 1.0]), np.array([o["loc"]])
                set_params(strict)
                conf.measure(rows, u, idx, loc); twin.measure(rows, u, idx, loc); ref.measure(None, u, _Table(rows, idx, loc))
                set_params(params)
                assert conf.N == twin.N == ref.N == N + 1
            elif kind == "pblock":
                r0, c0, nr, nc = o["r0"], o["c0"], o["nr"], o["nc"]
                bc, bt = conf.pblock(r0, c0, nr, nc), twin.get_P_block(r0, c0, nr, nc)
                Pr = ref.P
                agree(bc, bt, "P block", np.abs(Pr).max())
                to_oracle(bc, Pr[r0:r0 + nr, c0:c0 + nc], np.abs(Pr).max(), "P", "P block (configured)")
                to_oracle(bt, Pr[r0:r0 + nr, c0:c0 + nc], np.abs(Pr).max(), "P", "P block (twin)")
            elif kind == "diag":
                dc, dt, dr = conf.diag(), twin.get_P_diag_blocks(), diag_of(ref.P)
                sP = np.abs(ref.P).max()
                agree(dc, dt, "diagonal blocks", sP)
                to_oracle(dc, dr, sP, "P", "diagonal blocks (configured)")
                to_oracle(dt, dr, sP, "P", "diagonal blocks (twin)")
            elif kind == "shrink":
                n2 = 3 + 2 * o["N"]
                xc = conf.get_x()
                conf.shrink(np.ascontiguousarray(xc[:n2]))
                xt, Pt, stw = twin.get_x(), twin.get_P(), twin.get_s()
                twin.close()
                twin = fresh_twin()
                twin.set_state(xt[:n2], Pt[:n2, :n2], stw[:o["N"]])
                ref.set_state(ref.x[:n2], ref.P[:n2, :n2], ref.s[:o["N"]])
            elif kind == "lowrank":
                x, s, d, U = _lowrank_data(o["N"], o["seed"])
                conf.front.load_lowrank_state(x, s, d, U)
                twin.close()
                twin = fresh_twin()
                twin.load_lowrank_state(x, s, d, U)
                ref.set_state(x, np.diag(d) + U @ U.T, s)
            elif kind == "save":
                conf.save(o["tag"])
                twin.checkpoint_save(os.path.join(tmp, "twin_%d.ckpt" % o["tag"]))
                snaps[o["tag"]] = (ref.x, ref.P, ref.s)
            elif kind == "load":
                conf.load(o["tag"])
                twin.close()
                twin = fresh_twin()
                twin.checkpoint_load(os.path.join(tmp, "twin_%d.ckpt" % o["tag"]))
                ref.set_state(*snaps[o["tag"]])
            elif kind == "hint":
                conf.hint(o["k"])
            elif kind == "prefetch":
                conf.prefetch(o["ks"])
            elif kind == "prefetch_next":
                corr = []
                for c in o["corr"]:
                    z = obs(c["k"], c["nz"])
                    corr.append((z, Rz(z), c["k"]))
                    ref.correct(z, Rz(z), c["k"] + 1)
                conf.prefetch_next_block(o["ks"], corr)
                for z, R, k in corr:
                    twin.correct(z, R, k)
            kernels |= conf.kernels()
            if (i + 1) % cfg["cadence"] == 0:
                read()
                since_read = []
        read(full=True)
    except Exception as ex:      # (the original traceback stays attached as the cause)
        raise AssertionError("%s\nop %d; ops since the last agreeing read: %s\n%s: %s" % (
            what, i, since_read[-24:], type(ex).__name__, ex)) from ex
    finally:
        conf.close(); twin.close()
    hit = sorted({name for name, _ in kernels if name})
    full = sum(1 for name, pairs in kernels if name.startswith(cfg["kernel"]) and pairs == cfg["batch"])
    print("%s: %.2f s, worst vs oracle x %.2e P %.2e costs %.2e, vs twin %.2e, kernels %s" % (
        what, time.time() - t0, worst["x"], worst["P"], worst["cost"], worst["twin"], hit))
    # a launch of the full batch's kernel WITH a full batch of pairs (a partial flush may select the same instance)
    assert full, "%s: %s never ran with %d pairs (%s)" % (what, cfg["kernel"], cfg["batch"], sorted(kernels))


@pytest.mark.parametrize("seed", range(NSEEDS))
def test_random_schedule(seed, oracle_lib, tmp_path):
    run_seed(seed, str(tmp_path))
