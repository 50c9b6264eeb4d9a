// Fragment of kernels.hip (included there, inside its anonymous namespace, after factor_map.h, whose d4_t and kFactorBlock it uses): the
// pieces that the calls which treat P as a matrix share -- the draws (sample_map.h), the solves (solve_map.h) and the plain product
// (multiply_map.h).  Each piece exists once: chunk_k, tile_mac, segment_of, chunk_tree_sums.
#pragma once

// ---------------------------------------------------------------------------------------------------
// A CHUNK is kFactorChunk = 16 vectors, one a COLUMN (kernel_args.h: FactorSampleArgs), the N-width of v_mfma_f64_16x16x4_f64.
// THE PRODUCT OF A TILE WITH A CHUNK, entry (row i, vector c): a chain fma(A[i][k], x_c[k], acc) over k in chunk_k's order -- steps s
// ascending, the four terms t of a matrix instruction ascending: the instruction is a k-ordered chain of correctly rounded FMAs
// (flush64_mfma.h), and EKF_FACTOR_FMA_TWIN (the host builds of tests/support) compiles that chain entry by entry.  Where the chain
// starts (0, or the entry it updates), whether A is read transposed or negated (negation is exact) and which tiles follow one another
// in one chain is the caller's: sample_map.h, solve_map.h, multiply_map.h.
// THE SEGMENTS OF A TILE ROW: tile row I is cut into I / S + 1 segments of S tiles, one workgroup and one partial block each; the
// partial blocks of all tile rows lie one after another (factor_segment_base, kernel_args.h) and segment_of is its inverse.
// THE ROBOT ROWS: per tile row a 3 x 16 part (row q, vector c, at q * kFactorChunk + c); lane t of ONE workgroup of kFactorBlock lanes
// adds the parts of tile rows t, t + 256, .. ascending to 0 and the 256 sums of each of the 48 quantities meet in chunk_tree_sums'
// pairwise tree, the order of k_factor_finish's: a fixed order for a given number of tile rows.
// ---------------------------------------------------------------------------------------------------

// The k index of step s, term t.  Steps 2 p and 2 p + 1 of term t are the two ADJACENT doubles 8 p + 2 t and 8 p + 2 t + 1, one 16-byte
// load, and the four terms' loads of one row lie side by side: a load instruction of a wavefront reads 64 contiguous bytes of each of 16
// tile rows, and two of them in a row use every 128-byte line whole.  (k_factor_trail's factor_k gives a lane 16 contiguous doubles, so
// that each of its load instructions touches 64 lines for 16 bytes each; what either order cost the apply pass: DESIGN.md section 3x.)
__device__ __forceinline__ constexpr int chunk_k(int s, int t) { return 8 * (s >> 1) + 2 * t + (s & 1); }

// acc(16 rows from row0 of the product, column lc) += op(A) X, A a TF x TF tile, row-major, read as it stands (kTrans false) or transposed,
// negated or not; X the column lc of the staged chunk, TF entries in LDS.  Lane (lr, lc) = (lane / 16, lane % 16) supplies A(row lc, term
// lr) and X(term lr) and holds rows row0 + lr + 4 r.
template <int TF, bool kTrans, bool kNeg>
__device__ __forceinline__ void tile_mac(d4_t &acc, const double *__restrict__ A, const double *__restrict__ X, int row0, int lr, int lc) {
    constexpr int kSteps = TF / 4;
#if defined(EKF_FACTOR_FMA_TWIN)
    (void)lc;
    for (int r = 0; r < 4; ++r)
        for (int s = 0; s < kSteps; ++s)
            for (int t = 0; t < 4; ++t) {
                const int i = row0 + lr + 4 * r;
                const double v = kTrans ? A[chunk_k(s, t) * TF + i] : A[i * TF + chunk_k(s, t)];
                acc[r] = fma(kNeg ? -v : v, X[chunk_k(s, t)], acc[r]);
            }
#else
    double av[kSteps], bv[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const double v = kTrans ? A[chunk_k(s, lr) * TF + row0 + lc] : A[(row0 + lc) * TF + chunk_k(s, lr)];
        av[s] = kNeg ? -v : v;
    }
#pragma unroll
    for (int s = 0; s < kSteps; ++s) bv[s] = X[chunk_k(s, lr)];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#endif
}

// Segment w of a grid of factor_segment_base(nF, S) workgroups: tile row I, its segment seg, the tiles J0 .. J1 - 1.  Tile rows g S ..
// g S + S - 1 have g + 1 segments each, so g comes from a square root and the two loops put right a guess that is off by one.
__device__ __forceinline__ void segment_of(int64_t w, int S, int &I, int &seg, int &J0, int &J1) {
    int64_t g = (int64_t)((sqrt(8.0 * (double)w / S + 1.0) - 1.0) * 0.5);
    while (S * g * (g + 1) / 2 > w) --g;
    while (S * (g + 1) * (g + 2) / 2 <= w) ++g;
    const int64_t in = w - S * g * (g + 1) / 2;
    I = (int)(g * S + in / (g + 1));
    seg = (int)(in % (g + 1));
    J0 = seg * S;
    J1 = J0 + S <= I + 1 ? J0 + S : I + 1;
}

// sums[q * kFactorChunk + c] = the sum over the workgroup's kFactorBlock lanes of acc[q * kFactorChunk + c], by the pairwise tree in LDS;
// every lane of the workgroup calls it, and may read sums on return.
__device__ __forceinline__ void chunk_tree_sums(const double (&acc)[3 * kFactorChunk], double (&red)[kFactorChunk][kFactorBlock],
                                                double (&sums)[3 * kFactorChunk]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int c = 0; c < kFactorChunk; ++c) red[c][tid] = acc[q * kFactorChunk + c];
        __syncthreads();
        for (int off = kFactorBlock / 2; off > 0; off >>= 1) {
            if (tid < off)
                for (int c = 0; c < kFactorChunk; ++c) red[c][tid] = red[c][tid] + red[c][tid + off];
            __syncthreads();
        }
        if (tid < kFactorChunk) sums[q * kFactorChunk + tid] = red[tid][0];
        __syncthreads();
    }
}
