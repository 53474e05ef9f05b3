// gq_segment_body.inc -- the body of the K5 segment kernel (gq_gptq.hip), included once per __global__ wrapper: ONE text of the
// walk for gptq_segment_kernel<PERM, UNI, BANDS> and for gptq_segment_iq4_kernel.  The including function provides the names
// of gptq_segment_kernel's parameters, the compile-time flags PERM / UNI / BANDS / IQ4 and, under IQ4, `iq4tab`
// (iq4::BestReg).  It is a textual include and not an inlined device function because the four existing instantiations must
// keep their machine code instruction for instruction (DESIGN.md K28): as an always-inlined function template the same text
// compiled to slightly different schedules.
    // One workgroup = 64 rows (lane = row) x SEG_WAVES waves.  Wave 0 walks the columns (the dependent chain) one
    // 16-column sub-block ("tile") at a time; the rank-1 updates of the later tiles run UNDER the next chain:
    //   iteration t:  wave 0: chain(t) -> -err of tile t into ne[t & 1]
    //                 waves 1..7: apply ne[(t-1) & 1] (the errors of tile t-1) to the tiles t+1.. (deferred one tile)
    //                 barrier;  all 8 waves: apply ne[t & 1] to tile t+1 only, two columns each;  barrier
    // Tile u thus receives the errors of tiles 0, 1, .., u-2 (deferred, iterations 1..u-1) and then of tile u-1 (the
    // split step of iteration u-1), in this order, each as the same (mul, add) pairs in the same k order as the
    // reference's successive addr_ calls (gptq.py:267): results are unchanged, the update time leaves the critical
    // path (41 -> see DESIGN.md K5).
    extern __shared__ __attribute__((aligned(16))) float seg_smem[];
    float* wl = seg_smem;                   // wl[j*64 + lane]: working copy, column-major (32 KiB)
    float* Us = seg_smem + SEG * 64;        // Us[i*SEG + j] = U[a+i, a+j]: diagonal block (64 KiB), read back
                                            // with wave-uniform (broadcast) 16-byte LDS loads
    float* ne = Us + SEG * SEG;             // ne[(t & 1)*SB*64 + k*64 + lane]: -err of tile t, double-buffered (8 KiB)
    double* rdiag = reinterpret_cast<double*>(ne + 2 * SB * 64);  // rdiag[i] = 1 / U[a+i, a+i] in fp64 (1 KiB)
    // the group parameters of tile t for the row of `lane` (8 KiB): in registers they stayed live across all eight
    // tiles and, with U's rows hoisted over an unrolled tile loop, pushed wave 0's chain into scratch (DESIGN.md K5)
    double* rdg = rdiag + SEG;                                    // rdg[t*64 + lane] = 1 / max(ds, 1e-9) in fp64
    float* dsg = reinterpret_cast<float*>(rdg + SEG_NT * 64);     // dsg[t*64 + lane] = f32(d) * s
    float* dmg = dsg + SEG_NT * 64;                               // dmg[t*64 + lane] = f32(dmin) * m
    int64_t band_row0 = 0;  // BANDS: s / m are indexed by the row inside the band
    if constexpr (BANDS) {
        static_assert(!PERM && !UNI, "bands are K-quants in natural column order");
        const BandTable& bt = bands.t;
        int k = 0;
        while (k + 1 < bt.n && (int)blockIdx.x >= bt.end64[k]) ++k;
        const uint32_t info = bt.info[k];
        G = (int)(info & 0xffu);
        is_signed = (int)((info >> 8) & 1u);
        qmin = (float)(int8_t)((info >> 16) & 0xffu);
        qmax = (float)(info >> 24);
        band_row0 = k ? (int64_t)bt.end64[k - 1] * 64 : 0;
        s += bt.sm_off[k];
        m += bt.sm_off[k];
    }
    // The row's parameter arrays as per-lane pointers, formed once: the seven scalar arguments behind them need not stay
    // in SGPRs over both halves (VGPRs are plentiful here, SGPRs are not).
    const int64_t nsg = C / 256, ng = C / G;
    const int64_t prow = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63), pr = prow < R ? prow : 0;
    const uint16_t* const drow = UNI ? nullptr : d + pr * nsg;
    const uint16_t* const dminrow = UNI ? nullptr : dmin + pr * nsg;
    const uint8_t* const srow = UNI ? nullptr : s + (pr - band_row0) * ng;  // BANDS: the row inside the band
    const uint8_t* const mrow = UNI ? nullptr : m + (pr - band_row0) * ng;
    const float* const uscrow = UNI ? uscale + pr * ng : nullptr;
    const float* const uzrow = UNI ? uzero + pr * ng : nullptr;
    for (int half = 0; half < npair; ++half) {
    if (half) {  // the partner block: same rows, next 128 columns; the epilogue's stores of this workgroup are complete
        __syncthreads();
        a += SEG;
        src += SEG;
        err_col0 += SEG;
        Unext = nullptr;
    }
    // The thread's index is opaque per half: every predicate on it (row < R, tid < first, the epilogue's sixteen row
    // tests, ...) is invariant over this loop, and hoisted out of it the exec masks alone overflow the SGPR file.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    int lenq = len;  // the prologue's copy of len, opaque likewise (still wave-uniform): loop bounds and clamped offsets
    asm volatile("" : "+s"(lenq));
    const int lane = tid & 63, wid = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x * 64 + lane;
    const bool live = row < R;
    const int64_t r = live ? row : 0;
    // Two-step prologue: everything the FIRST tile's chain needs (U rows 0..15, the tile's 16 columns of W, its
    // reciprocal diagonal) is brought in by all waves, then the chain starts while waves 1..7 -- idle in
    // iteration 0 -- bring in the other 7/8 (gptq.py:225 w_blk = w[:, c1:c2].clone()).
    auto load_u_rows = [&](int i_lo, int i_hi, int t0, int nthr) {
        for (int idx = t0; idx < (i_hi - i_lo) * (SEG / 4); idx += nthr) {
            const int i = i_lo + idx / (SEG / 4), j4 = (idx % (SEG / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j4 < lenq) v = *reinterpret_cast<const float4*>(U + (a + i) * C + a + j4);
            *reinterpret_cast<float4*>(Us + i * SEG + j4) = v;
        }
    };
    auto load_w_cols = [&](int j_lo, int j_hi, int w0, int nw) {
        const float* sp = src + r * ld_src;
        for (int j = j_lo + w0 * 4; j < j_hi; j += 4 * nw) {
            float4 v = *reinterpret_cast<const float4*>(sp + j);
            wl[(j + 0) * 64 + lane] = v.x;
            wl[(j + 1) * 64 + lane] = v.y;
            wl[(j + 2) * 64 + lane] = v.z;
            wl[(j + 3) * 64 + lane] = v.w;
        }
    };
    const int first = lenq < SB ? lenq : SB;
    if (tid < first) rdiag[tid] = 1.0 / (double)U[(a + tid) * C + a + tid];
    load_u_rows(0, first, tid, SEG_WAVES * 64);
    load_w_cols(0, first, wid, SEG_WAVES);
    // group parameters of every tile of the segment, fetched before the chain starts (they do not depend on it): a
    // tile lies inside one group (16 | G), ds = f32(d) * s, dm = f32(dmin) * m, and 1 / max(ds, 1e-9) in fp64.  A lane
    // of wave 0 writes them and is the only one to read them back.
    // The segment lies inside one 256-column super-group (walk_block cuts it there), so d and dmin are read once; the
    // group of tile t is a / G + (a % G + 16 t) / G: one 64-bit division per segment, the eight others in 32 bits.
    // All loads are issued before the first value is used.
    constexpr int NT = SEG_NT;
    if constexpr (!PERM) {
        if (wid == 0) {
            const int64_t ga = a / G;
            const int ra = (int)(a - ga * G);
            float st[NT], mt[NT], dsup = 0.f, dminsup = 0.f;
            if constexpr (!UNI) {
                dsup = h2f(drow[a / 256]);
                dminsup = h2f(dminrow[a / 256]);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int64_t gi = ga + (ra + (t * SB < lenq ? t * SB : 0)) / G;
                if constexpr (UNI) {
                    st[t] = uscrow[gi];
                    mt[t] = uzrow[gi];
                } else {
                    st[t] = ival(srow[gi], is_signed);
                    mt[t] = ival(mrow[gi], is_signed);
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float dst = UNI ? st[t] : dsup * st[t], dmt = UNI ? mt[t] : dminsup * mt[t];
                dsg[t * 64 + lane] = dst;
                dmg[t * 64 + lane] = dmt;
                if constexpr (!IQ4) rdg[t * 64 + lane] = 1.0 / (double)(dst < 1e-9f ? 1e-9f : dst);  // quant_utils.py:37 clamp_min(eps)
            }
        }
    }
    __syncthreads();
    if (wid != 0) {  // under the first chain
        const int ht = tid - 64;
        if (ht >= first && ht < lenq) rdiag[ht] = 1.0 / (double)U[(a + ht) * C + a + ht];
        load_u_rows(first, lenq, ht, (SEG_WAVES - 1) * 64);
        load_w_cols(first, lenq, wid - 1, SEG_WAVES - 1);
    }

    // The tile loop stays rolled: unrolled, the compiler hoisted the wave-uniform reads of U's rows across tiles into
    // SGPRs and spilled both register files.  ntile is wave-uniform (a kernel argument), so all eight waves reach
    // every barrier of the loop and leave it together.
    const int ntile = len / SB;
#pragma unroll 1
    for (int t = 0; t < ntile; ++t) {
        const int i0 = t * SB;
        float* net = ne + (t & 1) * (SB * 64);
        if (wid == 0) {
            const int64_t col0 = a + i0;
            float ds = 0.f, dm = 0.f, dsv[PERM ? SB : 1], dmv[PERM ? SB : 1];
            double rden = 0.0, rdenv[PERM ? SB : 1];
            if constexpr (PERM) {
                // lane k & 15 looks up column k: one vector division by G for the tile, handed round by lane shuffles
                // (sixteen wave-uniform lookups are 32 scalar quotients alive at once -- they spilled the SGPR file)
                const int pcl = perm[col0 + (lane & (SB - 1))], sgl = pcl / 256, gl = pcl / G;
#pragma unroll
                for (int k = 0; k < SB; ++k) {
                    const int sg = __shfl(sgl, k), g = __shfl(gl, k);
                    dsv[k] = h2f(drow[sg]) * ival(srow[g], is_signed);
                    dmv[k] = h2f(dminrow[sg]) * ival(mrow[g], is_signed);
                    rdenv[k] = 1.0 / (double)(dsv[k] < 1e-9f ? 1e-9f : dsv[k]);
                }
            } else {
                ds = dsg[t * 64 + lane];
                dm = dmg[t * 64 + lane];
                if constexpr (!IQ4) rden = rdg[t * 64 + lane];
            }
            float wr[SB], nerr[SB], wq[SB];
            uint32_t qpack[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < SB; ++k) wr[k] = wl[(i0 + k) * 64 + lane];
#pragma unroll
            for (int k = 0; k < SB; ++k) {
                const float* urow = Us + (i0 + k) * SEG + i0;  // wave-uniform LDS address (broadcast)
                if constexpr (PERM) { ds = dsv[k]; dm = dmv[k]; rden = rdenv[k]; }
                float q;
                if constexpr (IQ4) {  // ds = step, dm = istep; the product step * kv[code] is exact (11 + 5 + 7 bits)
                    int code;
                    float kq;
                    iq4tab.best(dm * wr[k], code, kq);
                    q = (float)code;
                    wq[k] = ds * kq;
                } else if constexpr (UNI) {
                    q = clampf(rintf(div_rcp64(wr[k], rden) + dm), qmin, qmax);  // fast_obq.py:173, quant_utils.py:23-25
                    wq[k] = ds * (q - dm);                                       // :174, quant_utils.py:28-29
                } else {
                    q = clampf(rintf(div_rcp64(wr[k] + dm, rden)), qmin, qmax);  // gptq.py:247-254
                    wq[k] = dequantize1(q, ds, dm);                              // :255-261
                }
                const float err = div_rcp64(wr[k] - wq[k], rdiag[i0 + k]);                 // :264
                const uint8_t qb = is_signed ? (uint8_t)(int8_t)q : (uint8_t)q;
                qpack[k >> 2] |= (uint32_t)qb << (8 * (k & 3));
                // :267 addr_(err, U[i, i:], alpha=-1): self + (alpha*err)*u, two roundings
                const float nk = -err;
                nerr[k] = nk;
#pragma unroll
                for (int kk = k; kk < SB; ++kk) wr[kk] = wr[kk] + nk * urow[kk];
            }
            // published after the chain: an LDS store inside it would order every later LDS read of U behind it
            // (the compiler cannot tell that `ne` and `Us` never overlap)
#pragma unroll
            for (int k = 0; k < SB; ++k) net[k * 64 + lane] = nerr[k];
            if (live) {
                *reinterpret_cast<uint4*>(qweight + row * C + col0) =
                    make_uint4(qpack[0], qpack[1], qpack[2], qpack[3]);
                float* wp = W + row * C + col0;
                float* ep = Err + row * ld_err + err_col0 + i0;
#pragma unroll
                for (int k = 0; k < SB; k += 4) {
                    *reinterpret_cast<float4*>(wp + k) = make_float4(wq[k], wq[k + 1], wq[k + 2], wq[k + 3]);
                    *reinterpret_cast<float4*>(ep + k) =
                        make_float4(-nerr[k], -nerr[k + 1], -nerr[k + 2], -nerr[k + 3]);
                }
            }
        }
        // deferred: the errors of tile t-1 go into the tiles t+1.., 16 columns per helper wave and turn; each element
        // sees the same sequence of (mul, add) pairs, in the same order of i, as 16 successive addr_ calls
        // (packed v_pk_mul_f32 / v_pk_add_f32 were measured 35 % SLOWER here)
        if (wid != 0 && t > 0) {
            const float* nep = ne + ((t - 1) & 1) * (SB * 64);
            if (Unext != nullptr && wid == SEG_WAVES - 1) {
                // the epilogue wants all 128 (negated) errors of the block: tile t-1's go where its working columns were
                // (dead since its chain started), off the chain's wave
#pragma unroll
                for (int k = 0; k < SB; ++k) wl[(i0 - SB + k) * 64 + lane] = nep[k * 64 + lane];
            }
            int turn = 0;
            for (int j0 = i0 + SB; j0 < len; j0 += SB, ++turn) {
                if ((turn % (SEG_WAVES - 1)) + 1 != wid) continue;
                float wt[SB], nk[SB];
#pragma unroll
                for (int jj = 0; jj < SB; ++jj) wt[jj] = wl[(j0 + jj) * 64 + lane];
#pragma unroll
                for (int k = 0; k < SB; ++k) nk[k] = nep[k * 64 + lane];
#pragma unroll
                for (int k = 0; k < SB; ++k) {
                    const float* urow = Us + (i0 - SB + k) * SEG + j0;
#pragma unroll
                    for (int jj = 0; jj < SB; ++jj) wt[jj] = wt[jj] + nk[k] * urow[jj];
                }
#pragma unroll
                for (int jj = 0; jj < SB; ++jj) wl[(j0 + jj) * 64 + lane] = wt[jj];
            }
        }
        __syncthreads();
        // the next tile needs this tile's errors NOW: all eight waves, two of its columns each
        if (i0 + SB < len) {
            constexpr int CPW = SB / SEG_WAVES;
            const int j0 = i0 + SB + wid * CPW;
            float wt[CPW];
#pragma unroll
            for (int jj = 0; jj < CPW; ++jj) wt[jj] = wl[(j0 + jj) * 64 + lane];
#pragma unroll
            for (int k = 0; k < SB; ++k) {
                const float nk = net[k * 64 + lane];
#pragma unroll
                for (int jj = 0; jj < CPW; ++jj) wt[jj] = wt[jj] + nk * Us[(i0 + k) * SEG + j0 + jj];
            }
#pragma unroll
            for (int jj = 0; jj < CPW; ++jj) wl[(j0 + jj) * 64 + lane] = wt[jj];
        }
        __syncthreads();
    }
    // ---- epilogue (r03): this block's errors into the NEXT block's 128 columns (its partner in the 256-column
    // scale-search group), W[rows, a+128 ..] -= E[64 x 128] U[a .., a+128 ..], on the matrix cores: per element a
    // k-ordered fma chain from 0 and one subtraction, exactly what the separate rank-128 launch (gemm32_kernel, MODE 0)
    // computed -- here with the negated errors the kernel already keeps, sum' = -sum exactly, w + sum' = w - sum -- so
    // the launch, its gap and its W round trip disappear.  U's diagonal block in LDS is dead once the chains are through.
    if (Unext != nullptr) {
        for (int idx = tid; idx < SEG * (SEG / 4); idx += SEG_WAVES * 64) {
            const int i = idx / (SEG / 4), j4 = (idx % (SEG / 4)) * 4;
            *reinterpret_cast<float4*>(Us + i * SEG + j4) = *reinterpret_cast<const float4*>(Unext + (int64_t)i * C + j4);
        }
        __syncthreads();
        const int rb = (wid & 1) * 32, cb = (wid >> 1) * 32;  // 2 x 4 sub-tiles of 32 x 32, one per wave
        const int li = lane & 31, lk = lane >> 5;
        const float* nel = ne + ((ntile - 1) & 1) * (SB * 64);  // the last tile's errors never moved
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll 8
        for (int k0 = 0; k0 < SEG; k0 += 2) {
            const int k = k0 + lk;
            const float ev = (k < SEG - SB) ? wl[k * 64 + rb + li] : nel[(k - (SEG - SB)) * 64 + rb + li];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ev, Us[k * SEG + cb + li], acc, 0, 0, 0);
        }
        // all 16 loads in flight before the first store (written as `*p += acc` the compiler must keep every load behind
        // the previous store: 16 dependent HBM round trips, 12 us per block)
        const int64_t r0 = (int64_t)blockIdx.x * 64 + rb + 4 * lk;
        int64_t Cq = C;  // opaque like tid above: the row offsets ro * C are formed here, not kept in SGPRs all along
        asm volatile("" : "+s"(Cq));
        float* wp = W + r0 * Cq + a + SEG + cb + li;
        float wv[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ro = (e & 3) + 8 * (e >> 2);
            wv[e] = (r0 + ro < R) ? wp[(int64_t)ro * Cq] : 0.0f;
        }
        // s_waitcnt vmcnt(0), on every path: the loads above sit under row predicates, and on the path that skips the
        // matching store nothing waits for them -- the compiler then pays that wait at the top of the partner block's
        // chains, where it also covers the previous tile's global stores.  The first store needs the loads anyway.
        __builtin_amdgcn_s_waitcnt(0x0f70);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ro = (e & 3) + 8 * (e >> 2);
            if (r0 + ro < R) wp[(int64_t)ro * Cq] = wv[e] + acc[e];
        }
    }
    }  // half
