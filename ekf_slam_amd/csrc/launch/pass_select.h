// Which kernel instance a pass over P runs: a pure function of the tile shape, the pair count and what the work set offers.  Host code,
// nothing from HIP (tests/test_pass_select_cpu.py compiles it with g++); launch/passes.h launches what it returns and
// ekf_downdate_kernel_name reports PassInstance::name.  DESIGN.md section 3 has the table.
#pragma once
#include <stdio.h>

namespace ekf_pass {

enum Family {
    kInvalid,       // no pass kernel exists for this storage type and tile edge
    kSplit3,        // k_split_pairs + k_flush_split3<2>                        (flush32_split.h)
    kStrip32,       // k_flush_strip32<8>                                       (flush32_pipe.h)
    kMfma32,        // k_flush_mfma32<256, 4, 2, 3, early>                      (flush32_mfma.h)
    kMfma64,        // k_flush_mfma<TS, T, chunk, cols>                         (flush64_mfma.h)
    kDowndateW,     // k_downdate_w<TS, T, slab, xcd, rowpanel>                 (downdate.h)
    kDowndate,      // k_downdate<TS, T, slab>                                  (downdate.h)
};

struct PassQuery {
    int elt;                // bytes of a stored element: 8 (f64 tiles) or 4 (f32 tiles)
    int T;                  // tile edge
    int npairs;             // pairs the pass applies, >= 1
    int arith;              // cfg.pass_arith: 0 = F64, 1 = F32, 2 = SPLIT3
    bool xcd_list;          // the work set has its 8 per-XCD streams
    bool strip_list;        // ... and the strip work list (PassAux::segs)
    bool planes;            // the bf16 planes of the split arithmetic exist (PassAux::Kb3 / Gb3)
    bool next_row;          // a sharded handle wants the next correction's row-panel extracted (NextRow)
    int slab_override;      // EKF_DOWNDATE_SLAB / _SLAB_BATCH of a tuning build; 0 (and any value the tile edge does not accept): the default
};

// the scalar tuning knobs (kernels.h::ekf_tune_int), at the product's values
struct PassKnobs {
    bool flush_mfma = true;     // EKF_FLUSH_MFMA
    int mfma_switch = 30;       // EKF_FLUSH_MFMA_SWITCH: chunks of 4 pairs up to here, of 8 beyond (flush64_mfma.h)
    int half_max = 12;          // EKF_FLUSH_HALF_MAX
    bool pass_strip = true;     // EKF_PASS_STRIP
    bool flush_xcd = true;      // EKF_FLUSH_XCD
};

struct PassInstance {
    Family family;
    int elt, T;
    int slab;               // rows per workgroup of the VALU kernels (set for every family: the override moves nothing else)
    int chunk, cols;        // kMfma64: pairs per staged chunk, columns of a work item
    bool early;             // kMfma32: the tile is requested in front of the last chunk's matrix work
    bool xcd, rowpanel;     // kDowndateW: walks the per-XCD streams / also extracts the next row-panel
    char name[64];          // what ekf_downdate_kernel_name reports
};

// Granularity of the VALU kernels.  One pair: ONE pass per workgroup (each lane loads, updates and stores exactly one 16-byte
// piece of a tile row; a workgroup covers 4 KiB of a tile): 6.06 TB/s at 10k landmarks vs 5.49 TB/s for a whole
// 64x64 tile per workgroup (profiles/round1_tuning.md).  Several pairs: the G vectors are re-read from L2 once
// per workgroup and pair, so a taller slab amortises them.  EKF_DOWNDATE_SLAB / EKF_DOWNDATE_SLAB_BATCH (rows
// per workgroup for 1 pair / several pairs) and EKF_DOWNDATE_GRID (grid cap) are tuning hooks.
// Production tiles: T = 128 for f64 storage, T = 256 for f32 storage (one 1 KiB tile row per wave instruction,
// K wave-uniform); T = 16 / 32 (generic kernel) and T = 64 exist for small maps and tests.
struct SlabRule { int elt, T, one_pair, several; int accepted[4]; };      // accepted: what the override may name
constexpr SlabRule kSlabRules[] = {
    { 8, 16, 16, 16, {} },
    { 8, 32, 16, 16, { 32 } },
    { 8, 64, 8, 64, { 64, 32, 16, 8 } },
    { 8, 128, 4, 32, { 32, 16, 8, 4 } },
    { 4, 16, 16, 16, {} },
    { 4, 32, 32, 32, {} },
    { 4, 64, 64, 64, {} },                    // 16 lanes per row -> generic kernel
    { 4, 128, 8, 64, {} },                    // two rows per wave instruction
    { 4, 256, 4, 32, { 32, 16, 8, 4 } },
};

// rows per workgroup, or 0: no rule for this storage type and tile edge
inline int pass_slab(const PassQuery &q) {
    for (const SlabRule &r : kSlabRules) {
        if (r.elt != q.elt || r.T != q.T) continue;
        for (int s : r.accepted) if (s != 0 && s == q.slab_override) return s;
        return q.npairs > 1 ? r.several : r.one_pair;
    }
    return 0;
}

inline PassInstance select_pass(const PassQuery &q, const PassKnobs &k = PassKnobs()) {
    PassInstance p = {};
    p.family = kInvalid; p.elt = q.elt; p.T = q.T; p.slab = pass_slab(q);
    if (p.slab == 0) return p;
    const char *ts = q.elt == 8 ? "double" : "float";
    const int np = q.npairs;
    const bool xcd = k.flush_xcd && q.xcd_list;
    // The matrix-core passes exist for the production shapes only.  F32 tiles: also for a single pair -- the 64 x 128 work items stream
    // the float tiles faster than the one-pair VALU kernel (40 k landmarks: 4.4 ms vs 4.9 ms per pass); F64 tiles: the one-pair VALU
    // kernel is the faster one (0.53 vs 0.56 ms)
    const bool have_mfma = (q.elt == 8 && q.T == 128) || (q.elt == 4 && q.T == 256);
    const int min_pairs = q.elt == 4 ? 1 : 2;
    if (have_mfma && xcd && k.flush_mfma && np >= min_pairs) {
        if (q.elt == 4) {
            if (q.arith == 2 && np >= 28 && np <= 64 && q.strip_list && q.planes) {
                // cfg.pass_arith = EKF_ARITH_SPLIT3, 28-64 pairs (below, the F32 kernels are the faster ones: 20 pairs 4.27 against 4.75 ms at
                // 40 000 landmarks, 32 pairs 5.08 against 4.74 -- round4_tuning.md 57): the float copies cut into three bf16 planes (logical
                // pair order, zeros beyond npairs), then the strip form of the pass on the bf16 matrix pipe (flush32_split.h) -- bound by
                // HBM, not by the matrix pipe
                p.family = kSplit3;
                snprintf(p.name, sizeof p.name, "k_flush_split3<2>");
                return p;
            }
            if (k.pass_strip && q.arith == 1 && np > 56 && np <= 64 && q.strip_list) {
                // 57-64 pairs (eight stages of eight): the strip form -- one persistent workgroup per CU walks row strips with -K in its
                // wavefronts' registers and a whole item's G double-buffered in LDS (flush32_pipe.h): 7.3 ms against 8.1-8.3 at 40 000
                // landmarks and 64 pairs, same bits
                p.family = kStrip32;
                snprintf(p.name, sizeof p.name, "k_flush_strip32<8>");
                return p;
            }
            if (q.arith >= 1 && np > 2) {
                // cfg.pass_arith = EKF_ARITH_F32 (and EKF_ARITH_SPLIT3 up to 27 pairs): the f32 matrix pipe (one or two pairs: the pass is
                // purely HBM-bound and the F64-arithmetic kernel below streams it 5 % faster, 4.0 against 4.3 ms at 40 k).
                // Three wavefronts per SIMD; from five pairs on the tile is requested in front of the LAST chunk's matrix work instead of
                // after it (its 64 registers are free once nothing is fetched any more): 5.37 against 5.63-5.67 ms at 32 pairs, 4.07
                // against 4.11-4.20 at 12, equal at 64 (profiles/round3_tuning.md 40)
                p.family = kMfma32;
                p.early = np > 4;
                snprintf(p.name, sizeof p.name, "k_flush_mfma32<%d,4,2,3%s>", q.T, p.early ? ",early" : "");
                return p;
            }
        }
        p.family = kMfma64;
        if (q.elt == 8 && np <= k.half_max) {
            // Up to 12 pairs the pass is HBM-bound and gains from finer work items: 64 rows x 64 columns (32 KiB, 4 accumulator blocks per
            // wavefront, five wavefronts per SIMD) -- 0.543 against 0.566 ms at 2-8 pairs, 10 000 landmarks; from ~16 pairs on the
            // 128-column items win (G is read from L2 once per 128 instead of 64 columns: 20 pairs 0.554 against 0.564).
            // profiles/round3_tuning.md 37.
            p.chunk = 4; p.cols = 64;
            snprintf(p.name, sizeof p.name, "k_flush_mfma<double,%d,4,64>", q.T);
            return p;
        }
        p.chunk = np <= k.mfma_switch ? 4 : 8; p.cols = 128;
        snprintf(p.name, sizeof p.name, "k_flush_mfma<%s,%d,%d>", ts, q.T, p.chunk);
        return p;
    }
    // a tile row of 64 or 32 lanes (16 bytes each): the wavefront-per-row kernel; narrower tiles: the generic one
    const int lanes = q.T / (16 / q.elt);
    if (lanes != 64 && lanes != 32) {
        p.family = kDowndate;
        snprintf(p.name, sizeof p.name, "k_downdate<%s,%d,%d>", ts, q.T, p.slab);
        return p;
    }
    p.family = kDowndateW;
    p.xcd = np > 1 && xcd;
    p.rowpanel = !p.xcd && q.next_row && np == 1;
    snprintf(p.name, sizeof p.name, "k_downdate_w<%s,%d,%d,%s%s>", ts, q.T, p.slab, p.xcd ? "true" : "false", p.rowpanel ? ",+rowpanel" : "");
    return p;
}

}  // namespace ekf_pass
