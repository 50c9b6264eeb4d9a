"""Seeded operation plans for tests/test_random_schedules_gpu.py (host only: no GPU, no library).

`plan(seed)` returns (cfg, ops): the seed's engine configuration and its list of op records, a pure function of the seed, so that a
failing seed can be printed and replayed.  The configuration is stratified, not drawn: `config(seed)` walks a fixed table so that 64
seeds cover every pass kernel a full batch can select (csrc/launch/pass_select.h: ekf_pass::select_pass), crossed with the asynchronous
pass, the shard layouts, the association modes and the association weight.

Configuration table (ROWS): storage, tile edge, the batches of the row, and the name prefix of the pass kernel a full batch selects.

  storage     tile        batches        pass kernel of a full batch
  f64         128         1              k_downdate_w<double,128,4,false>      (the one-pair VALU pass)
  f64         128         2-12           k_flush_mfma<double,128,4,64>
  f64         128         13-30          k_flush_mfma<double,128,4>
  f64         128         31-64          k_flush_mfma<double,128,8>
  f64         16 / 32     12-64          k_downdate<double,T,16>               (many-pair generic pass)
  f64         64          12-64          k_downdate_w<double,64,64,true>
  f32         256         1, 8 / 40, 64  k_flush_mfma<float,256,4> / <float,256,8>  (F64 arithmetic on float tiles)
  f32         16          5, 20          k_downdate<float,16,16>
  f32         128         1 / 5, 20      k_downdate_w<float,128,8,false> / <float,128,64,true>
  f32_mixed   256         1-2            k_flush_mfma<float,256,4>             (one or two pairs keep the F64-arithmetic pass)
  f32_mixed   256         3-4            k_flush_mfma32<256,4,2,3>
  f32_mixed   256         5-56           k_flush_mfma32<256,4,2,3,early>
  f32_mixed   256         57-64          k_flush_strip32<8>
  f32_split   256         28-64          k_flush_split3<2>

ekf_create refuses pass_arith F32 / SPLIT3 (f32_mixed, f32_split) on F64 storage or on a tile edge other than 256, and tile 256 on F64
storage: no row uses those.  Every other combination of the table with async {off, on}, shards {1, 2, 3, 4, 1-rank communicator},
device_assoc {0..3} and w_pos {0, 1} is accepted.  Calls with narrower preconditions are planned only where they hold: ekf_prefetch_next
needs batch > 1, a synchronous flush and F64 pass arithmetic; ekf_hint_next matters on sharded handles at batch 1 only.

Op records are dicts; "op" names the kind:
  predict {u}; correct {k, nz, local}; append {pos}; associate {k, nz, sig, costs}; measure {ks, nz, loc}; pblock {r0, c0, nr, nc};
  diag; shrink {N} (ekf_set_x with a prefix of x); lowrank {N, seed}; save {tag}; load {tag}; hint {k}; prefetch {ks};
  prefetch_next {ks, corr} (the announcement and the corrections that complete the current batch, one block).
`nz` are standard-normal draws: the runner turns them into noise on observations it computes from the oracle's x.
"""
import numpy as np

# storage, tile choices, batch choices (drawn per seed), expected-kernel rule
ROWS = [
    ("f64", (128,), (1,)),
    ("f64", (128,), tuple(range(2, 13))),
    ("f64", (128,), tuple(range(13, 31))),
    ("f64", (128,), tuple(range(31, 65))),
    ("f64", (16, 32, 64), tuple(range(12, 65))),
    ("f32", (256,), (1, 8, 40, 64)),
    ("f32", (16, 128), (1, 5, 20)),
    ("f32_mixed", (256,), (1, 2)),
    ("f32_mixed", (256,), (3, 4)),
    ("f32_mixed", (256,), tuple(range(5, 57))),
    ("f32_mixed", (256,), tuple(range(57, 65))),
    ("f32_split", (256,), tuple(range(28, 65))),
]
SHARDS = (1, 2, 3, 4, "comm")
ASSOC = (3, 1, 2, 0)
CADENCE = (1, 4, 16)
NSEEDS = 64
# ops after which no pair is pending (the library flushed, or replaced the state; prefetch_next's block ends on a batch boundary)
FLUSHING = {"pblock", "shrink", "lowrank", "save", "load", "prefetch_next"}
# ops a full-batch stretch must not contain: the flushes, and the ops that read or decide on the device (measure, associate)
STRETCH_BREAK = FLUSHING | {"measure", "associate"}


def expected_kernel(storage, tile, batch):
    """Name prefix of the pass kernel a full batch of `batch` pairs selects (csrc/launch/pass_select.h: ekf_pass::select_pass;
    tests/test_pass_select_cpu.py holds the two together)."""
    if storage == "f64":
        if tile == 128:
            if batch == 1:
                return "k_downdate_w<double,128,4,false"
            return "k_flush_mfma<double,128,4,64>" if batch <= 12 else "k_flush_mfma<double,128,4>" if batch <= 30 else \
                "k_flush_mfma<double,128,8>"
        if tile == 64:
            return "k_downdate_w<double,64,64,true>" if batch > 1 else "k_downdate_w<double,64,8,false"
        return "k_downdate<double,%d,16>" % tile
    if tile == 16:
        return "k_downdate<float,16,16>"
    if tile == 128:
        return "k_downdate_w<float,128,64,true>" if batch > 1 else "k_downdate_w<float,128,8,false"
    if storage == "f32_split" and batch >= 28:
        return "k_flush_split3<2>"
    if storage in ("f32_mixed", "f32_split") and batch > 2:
        return "k_flush_strip32<8>" if batch > 56 else "k_flush_mfma32<256,4,2,3>" if batch <= 4 else "k_flush_mfma32<256,4,2,3,early>"
    return "k_flush_mfma<float,256,%d>" % (4 if batch <= 30 else 8)


def config(seed):
    """The seed's configuration: a fixed walk over ROWS x async x shards x device_assoc x w_pos (within every row: both async values,
    all five shard layouts, all four association modes, both weights each with async off and on), the batch, tile and map size drawn
    inside the row."""
    rng = np.random.default_rng(7100 + seed)
    nrow = len(ROWS)
    storage, tiles, batches = ROWS[seed % nrow]
    batch = int(batches[(seed // nrow) * 7 % len(batches)]) if len(batches) > 1 else batches[0]
    if seed % nrow == 5 and seed // nrow < 4:             # f32 tile 256: 1, 8, 40, 64 in turn
        batch = batches[seed // nrow]
    tile = int(tiles[(seed // nrow) % len(tiles)])
    if storage == "f32" and tile == 16 and batch == 1:    # a one-pair pass on a map this small runs inside the gather (fused): use 128
        tile = 128
    # j: the seed's turn within its row (5 or 6 turns per row).  async alternates with j; the association mode and weight are drawn from
    # j shifted by the row, so that every row meets all four modes and both weights, each weight with async off and on
    j, r = seed // nrow, seed % nrow
    asy = bool(j % 2)
    shards = SHARDS[(seed + j) % len(SHARDS)]
    assoc = ASSOC[(j + r) % len(ASSOC)]
    w_pos = float((j // 2 + r) % 2)
    cadence = CADENCE[(seed // 5) % len(CADENCE)]
    half = tile // 2                                      # landmarks per tile row
    if tile == 256:
        lo = 130 if batch == 1 else 100                   # (above 128 landmarks: a one-pair pass is not fused into the gather)
        if (seed + seed // nrow) % 2 == 0:             # half the seeds: 1-8 landmarks below a multiple of 128
            N0 = int(128 * rng.integers((lo + 8) // 128 + 1, 700 // 128 + 1) - rng.integers(1, 9))
        else:
            N0 = int(rng.integers(lo, 701))
    elif tile == 128:
        lo = 130 if batch == 1 else 40
        N0 = int(64 * rng.integers(lo // 64 + 1, 400 // 64 + 1) + rng.integers(-8, 4))
        N0 = max(lo, min(400, N0))
    else:
        N0 = int(rng.integers(3, 121))
    return dict(seed=seed, storage=storage, tile=tile, batch=batch, async_flush=asy, shards=shards, device_assoc=assoc, w_pos=w_pos,
                cadence=cadence, N0=N0, cap=N0 + 40, half=half, kernel=expected_kernel(storage, tile, batch))


def describe(cfg):
    return "seed %d: storage %s tile %d batch %d async %s shards %s assoc %d w_pos %g N0 %d cadence %d" % (
        cfg["seed"], cfg["storage"], cfg["tile"], cfg["batch"], cfg["async_flush"], cfg["shards"], cfg["device_assoc"], cfg["w_pos"],
        cfg["N0"], cfg["cadence"])


class _Planner:
    def __init__(self, cfg, rng):
        self.c, self.rng = cfg, rng
        self.N = cfg["N0"]
        self.newest = self.N - 1
        self.since = 0            # corrections since the last batch boundary or flush
        self.ops = []
        self.saved = None         # tag of the open delayed checkpoint
        self.sharded = cfg["shards"] != 1
        self.nhint = cfg["seed"] // 12         # (right and wrong hints alternate across seeds too)

    def f(self, lo=0.0, hi=1.0):
        return float(self.rng.uniform(lo, hi))

    def nz(self):
        return [float(v) for v in self.rng.normal(size=2)]

    def edge_k(self):
        """A corrected landmark biased to the edges of the map: 0, N-1, the first / last landmark of a tile row, the newest append."""
        N, half = self.N, self.c["half"]
        r = self.rng.integers(0, 6)
        if r == 0:
            return 0
        if r == 1:
            return N - 1
        if r == 2 and 0 <= self.newest < N:
            return self.newest
        if r in (3, 4):
            row = int(self.rng.integers(0, (N + half - 1) // half))
            k = row * half + (0 if r == 3 else half - 1)
            return min(k, N - 1)
        return int(self.rng.integers(0, N))

    def add(self, op, **kw):
        kw["op"] = op
        self.ops.append(kw)
        if op in FLUSHING:
            self.since = 0
        elif op == "measure":             # its rows of known landmarks are corrections (the signature names the landmark)
            self.since = (self.since + len(kw["ks"])) % self.c["batch"]

    def predict(self):
        self.add("predict", u=[self.f(0, .3), self.f(-8, 8)])

    def correct(self, k=None, local=False):
        self.add("correct", k=self.edge_k() if k is None else int(k), nz=self.nz(), local=bool(local))
        self.since += 1
        if self.since >= self.c["batch"]:
            self.since = 0

    def append(self):
        if self.N >= self.c["cap"]:
            return False
        self.add("append", pos=[self.f(-15, 15), self.f(-15, 15)])
        self.newest = self.N
        self.N += 1
        return True

    def stretch(self, appends):
        """>= batch corrections with no flushing op in between (predicts, appends, diag reads only): at least one full batch."""
        n = self.c["batch"] + int(self.rng.integers(1, 4))
        where = set(int(v) for v in self.rng.integers(0, n, size=appends))
        for i in range(n):
            if self.rng.random() < 0.3:
                self.predict()
            if i in where:
                self.append()
            if self.rng.random() < 0.05:
                self.add("diag")
            self.correct()

    def reload_target_below(self):
        """N' < N: a tile-row edge below N minus 1-4 landmarks (appends cross it again) or anywhere below."""
        half = self.c["half"]
        edges = [e for e in range(half, self.N, half) if e - 4 >= 1]
        if edges and self.rng.random() < 0.7:
            return int(edges[int(self.rng.integers(0, len(edges)))] - self.rng.integers(1, 5))
        return int(self.rng.integers(1, self.N))

    def random_op(self):
        c = self.c
        kinds = ["predict", "correct", "correct", "append", "associate", "measure", "pblock", "diag"]
        p = [.2, .25, .2, .1, .08, .05, .05, .07]
        if self.sharded and c["batch"] == 1:
            kinds.append("hint"); p.append(.15)
        p = np.array(p) / sum(p)
        kind = kinds[int(self.rng.choice(len(kinds), p=p))]
        if kind == "predict":
            self.predict()
        elif kind == "correct":
            self.correct()
        elif kind == "append":
            self.append()
        elif kind == "associate":
            self.add("associate", k=self.edge_k(), nz=self.nz(), sig=int(self.rng.integers(1, self.N + 1)),
                     costs=bool(self.rng.integers(0, 2)))
        elif kind == "measure" and self.N + 1 < c["cap"]:
            self.measure()
        elif kind == "pblock":
            n = 3 + 2 * self.N
            r0 = int(self.rng.integers(0, n - 1)); c0 = int(self.rng.integers(0, n - 1))
            self.add("pblock", r0=r0, c0=c0, nr=int(self.rng.integers(1, min(9, n - r0) + 1)), nc=int(self.rng.integers(1, min(9, n - c0) + 1)))
        elif kind == "diag":
            self.add("diag")
        elif kind == "hint":
            # the hint names the landmark of the correction AFTER the next one (the next one's pass extracts its row-panel)
            k = self.edge_k()
            self.nhint += 1                               # right and wrong hints in turn
            self.add("hint", k=k if self.nhint % 2 else (k + 1) % self.N)
            self.correct()
            self.correct(k)

    def measure(self):
        """a scan: rows of 1-3 known landmarks (corrected) and one row that matches nothing (appended)"""
        m = int(self.rng.integers(1, 4))
        self.add("measure", ks=[self.edge_k() for _ in range(m)], nz=[self.nz() for _ in range(m)],
                 loc=[self.f(-15, 15), self.f(-15, 15)])
        self.newest = self.N
        self.N += 1

    def make_room(self, m):
        """a plain shrink (ekf_set_x) when fewer than m landmarks of capacity are left"""
        if self.N > self.c["cap"] - m:
            self.add("shrink", N=max(1, min(self.reload_target_below(), self.c["cap"] - m - 1)))
            self.N = self.ops[-1]["N"]
            self.newest = -1

    def shrink(self):
        if self.N < 2:
            self.append()
        self.add("shrink", N=self.reload_target_below())
        self.N = self.ops[-1]["N"]
        self.newest = -1
        self.grow(self.c["half"] // 2 if self.c["half"] <= 8 else 5)

    def lowrank(self, up):
        if up:
            self.make_room(8)
            N2 = int(self.rng.integers(self.N + 1, self.c["cap"] - 5))
        else:
            if self.N < 2:
                self.append()
            N2 = self.reload_target_below()
        self.add("lowrank", N=N2, seed=int(self.rng.integers(0, 2 ** 31)))
        self.N = N2
        self.newest = -1
        self.grow(5)

    def grow(self, m):
        """m appends between corrections right after a reload: across the tile-row edge the reload went below, if there is one."""
        for _ in range(m):
            if self.append():
                self.correct(self.N - 1)

    def prefetch(self):
        """prefetch_rows of up to `batch` landmarks, then corrections that run past the batch boundary: on groups the ones before it
        (on prefetched landmarks) go without an exchange (correct_local); a communicator handle lets the library decide."""
        m = int(self.rng.integers(1, min(self.c["batch"], 4) + 1))
        ks = sorted(set(self.edge_k() for _ in range(m)))
        self.add("prefetch", ks=ks)
        left = self.c["batch"] - self.since               # corrections up to and including the one that completes the batch
        for i in range(left + 2):
            k = ks[i % len(ks)] if i < left else self.edge_k()
            self.correct(k, local=i < left)

    def prefetch_next(self):
        """ekf_prefetch_next during a batch: the announcement and the corrections that complete the batch (one block), then
        corrections on the announced landmarks (local on groups: the prefetch holds until the next boundary)."""
        if self.since == 0:
            self.correct()
        m = int(self.rng.integers(1, min(self.c["batch"], 4) + 1))
        ks = sorted(set(self.edge_k() for _ in range(m)))
        corr = [dict(k=self.edge_k(), nz=self.nz()) for _ in range(self.c["batch"] - self.since)]
        self.add("prefetch_next", ks=ks, corr=corr)
        self.since = 0
        for i in range(min(len(ks) + 1, self.c["batch"] - 1)):
            self.correct(ks[i % len(ks)], local=True)


def plan(seed):
    """(cfg, ops) of a seed; see the module docstring."""
    cfg = config(seed)
    rng = np.random.default_rng(424242 + 1000 * seed)
    pl = _Planner(cfg, rng)
    length = max(60, 3 * cfg["batch"] + 20)
    sharded, batch = cfg["shards"] != 1, cfg["batch"]
    # the reloads and the calls with preconditions this seed makes, in a seeded order; two full-batch stretches among them
    events = ["stretch_a", "stretch_b", "shrink", "lowrank_down", "lowrank_up", "save", "load", "measure"]
    if seed % 3 == 0:
        events.append("lowrank_up" if seed % 2 else "lowrank_down")
    if sharded:
        events.append("prefetch")
        if batch > 1 and not cfg["async_flush"] and cfg["storage"] in ("f64", "f32"):
            events.append("prefetch_next")
    order = [events[i] for i in rng.permutation(len(events))]
    # the first stretch before any reload (the full batch's kernel runs at the seed's starting size); the load is the next event after
    # the save, so that only growth lies between them: the checkpoint always loads into a handle that has grown since the save
    order.remove("stretch_a"); order.insert(0, "stretch_a")
    order.remove("load"); order.insert(order.index("save") + 1, "load")
    budget = max(length - 2 * (batch + 4) - 12 * len(order), 24)
    gaps = rng.multinomial(budget, np.ones(len(order) + 1) / (len(order) + 1))
    for ev, gap in zip(order + [None], gaps):
        for _ in range(int(gap)):
            pl.random_op()
        if ev is None:
            break
        if ev.startswith("stretch"):
            pl.stretch(appends=1 + int(rng.integers(0, 3)))
        elif ev == "shrink":
            pl.shrink()
        elif ev.startswith("lowrank"):
            pl.lowrank(ev == "lowrank_up")
        elif ev == "save":
            pl.make_room(4)
            pl.add("save", tag=len(pl.ops))
            pl.saved = pl.ops[-1]["tag"]
            for _ in range(3):                            # keep going, appends included: the load finds a larger handle
                pl.append(); pl.correct()
        elif ev == "load":
            pl.add("load", tag=pl.saved)
            pl.N = landmark_counts(cfg, pl.ops[:pl.saved])[-1]
            pl.newest = -1
            pl.grow(4)
        elif ev == "measure":
            pl.make_room(3)
            pl.measure()
        elif ev == "prefetch":
            pl.prefetch()
        elif ev == "prefetch_next":
            pl.prefetch_next()
    while len(pl.ops) < length:
        pl.random_op()
    return cfg, pl.ops


def landmark_counts(cfg, ops):
    """N before each op (and after the last): what the runner will see."""
    N, out, saves = cfg["N0"], [], {}
    for o in ops:
        out.append(N)
        k = o["op"]
        if k in ("append", "measure"):
            N += 1
        elif k in ("shrink", "lowrank"):
            N = o["N"]
        elif k == "save":
            saves[o["tag"]] = N
        elif k == "load":
            N = saves[o["tag"]]
    out.append(N)
    return out


def full_batch_stretches(cfg, ops):
    """Maximal runs of ops without a flushing, reading or deciding op (STRETCH_BREAK): the number of corrections in each (a run of r
    holds r // batch full batches)."""
    runs, cur = [], 0
    for o in ops:
        if o["op"] in STRETCH_BREAK:
            runs.append(cur); cur = 0
        elif o["op"] == "correct":
            cur += 1
    runs.append(cur)
    return runs

