// The body of k_f4096 and k_f4096_fine (fdc_fused4096.hip), included once in each: the kernel without fine tuning is the text it always was (FINE = false
// discards the rest), so its instructions do not depend on how the FINE forms are built.  In scope: the kernel's arguments, FINE, ROWS, and fa (F4Fine).
// sample T of row A: the store the kernel always had; FINE: the value turned first (before oq_bits for integer TO)
#define F4_PUT(A, T, V, FB, FS) out_st(out + A.dst + T, fine_val<FINE>(V, FB, FS, T), oq_scale)
    static_assert(!ROWS || std::is_same<TO, float2>::value, "integer output: not the waterfall form");
    static_assert(!ROWS || !FINE, "fine tuning: not the waterfall form");
    [[maybe_unused]] cf fb0 = mk(1.0f, 0.0f), fb1 = mk(1.0f, 0.0f);        // FINE: the bases and step factors of the wave's one or two rows per lane
    [[maybe_unused]] const float2 *fs0 = nullptr, *fs1 = nullptr;
    [[maybe_unused]] const float iq_scale = iq_tail_scale(wf);
    [[maybe_unused]] const float oq_scale = oq_tail_scale(wf);
    float2 *tiles = reinterpret_cast<float2 *>(fdc_smem_f4);
    float2 *t256 = reinterpret_cast<float2 *>(fdc_smem_f4 + f4_off_t256(TEAMS));
    float2 *t4k = reinterpret_cast<float2 *>(fdc_smem_f4 + f4_off_t4k(TEAMS));
    const F4Row *srows = reinterpret_cast<const F4Row *>(fdc_smem_f4 + f4_off_rows(TEAMS));
    const int team = TEAMS == 1 ? 0 : threadIdx.x >> 8, tid = threadIdx.x & 255, lo = tid & 15, hi = tid >> 4;
    // neighbouring blocks share R - 1 of R input samples: workgroup ids go round the eight XCDs, so XCD x takes the x-th eighth of the launch
    // and the shared samples are hits in ITS L2
    const int ngroups = (nb + TEAMS - 1) / TEAMS, per = (ngroups + 7) >> 3;
    const int grp = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (grp >= ngroups) return;
    const int m0 = TEAMS * grp, m = m0 + team;
    float2 *tile = tiles + team * kF4TilePts;
    if (team == 0) {
        t256[hi * 18 + lo] = tw[((16 * hi * lo) & 4095) * twstride];
        t4k[hi * 18 + lo] = tw[(hi * lo) * twstride];
    }
    if (team == TEAMS - 1) {
        if (tid < 64 * TEAMS) reinterpret_cast<float4 *>(fdc_smem_f4 + f4_off_rows(TEAMS))[tid] = reinterpret_cast<const float4 *>(rows)[tid];
        if constexpr (WIDE) {
            float2 *w1k = reinterpret_cast<float2 *>(fdc_smem_f4 + f4_off_w1k(TEAMS)), *w64 = reinterpret_cast<float2 *>(fdc_smem_f4 + f4_off_w64(TEAMS));
            for (int i = tid; i < 512; i += 256) w1k[(i >> 5) * 34 + (i & 31)] = tw[((i >> 5) * (i & 31)) * (4 * twstride)];
            if (tid < 64) w64[(tid >> 5) * 34 + (tid & 31)] = tid < 32 ? make_float2(1.0f, 0.0f) : tw[(tid & 31) * (64 * twstride)];
        }
    }
    // ---- forward transform: n = a + 16 b + 256 c, k = k0 + 16 k1 + 256 k2 (k_fft4096, fdc_chanwide.hip) ---------------------------------
    cf v[32];
    {
        cf (&u)[16] = reinterpret_cast<cf (&)[16]>(v[0]);
        // integer input: the sixteen raw words first, all in flight together; widened behind the barrier (converted one by one as they
        // arrive, the compiler waited for each load before issuing the next)
        [[maybe_unused]] unsigned raw[16];
        if constexpr (!std::is_same<TI, float2>::value) {
#pragma unroll
            for (int c = 0; c < 16; c++) raw[c] = m < nb ? iq_bits(in + (size_t)m * in_stride + (tid + 256 * c)) : 0u;
        } else
#pragma unroll
        for (int c = 0; c < 16; c++) u[c] = m < nb ? ld2(in + ((size_t)m * in_stride + (tid + 256 * c))) : mk(0.f, 0.f);
        __syncthreads();
        if constexpr (!std::is_same<TI, float2>::value) {
#pragma unroll
            for (int c = 0; c < 16; c++) u[c] = iq_widen_bits(TI{}, raw[c], iq_scale);
        }
        dft16<false>(u);                                             // layer 1 over c: k0 in u[rev16(k0)]; thread = (a = lo, b = hi)
        {
            cf w[16];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const float4 t = ld4(&t256[hi * 18 + 2 * i]);
                w[2 * i] = mk(t.x, t.y); w[2 * i + 1] = mk(t.z, t.w);
            }
#pragma unroll
            for (int k0 = 0; k0 < 16; k0++) st2(&tile[k0 * 272 + tid], k0 == 0 ? u[rev16(0)] : cmul(u[rev16(k0)], w[k0]));
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 16; b++) u[b] = ld2(&tile[hi * 272 + b * 16 + lo]);      // thread = (a = lo, k0 = hi)
        dft16<false>(u);                                             // layer 2 over b: k1 in u[rev16(k1)]
        __syncthreads();                                             // every read of exchange 1 is done
        {
            const cf s = ld2(&t4k[lo * 18 + hi]);                    // W_4096^(a k0)
            cf w[16];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const float4 t = ld4(&t256[lo * 18 + 2 * i]);        // W_256^(a k1)
                w[2 * i] = mk(t.x, t.y); w[2 * i + 1] = mk(t.z, t.w);
            }
#pragma unroll
            for (int k1 = 0; k1 < 16; k1++) st2(&tile[k1 * 257 + hi * 16 + (lo ^ hi)], cmul(u[rev16(k1)], k1 == 0 ? s : cmul(s, w[k1])));
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 16; a++) u[a] = ld2(&tile[hi * 257 + lo * 16 + (a ^ lo)]);   // thread = (k0 = lo, k1 = hi)
        dft16<false>(u);                                             // layer 3 over a: bin k0 + 16 k1 + 256 k2 in u[rev16(k2)]
        __syncthreads();                                             // every read of exchange 2 is done
        // the shifted spectrum (fftshift: bin k at k + N/2; python/FrequencyDomainChannelizer.py:206 fft_vcc(..., shift = True)), times 1/N
#pragma unroll
        for (int k2 = 0; k2 < 16; k2++) st2(&tile[tid + 256 * (k2 ^ 8)], u[rev16(k2)] * (1.0f / 4096.0f));
        if constexpr (ROWS) {
            // shifted bin tid + 256 (k2 ^ 8) is pixel (tid >> 2) + 64 (k2 ^ 8): the four bins of a pixel are in four adjacent lanes (one DPP quad);
            // m is uniform over the team, so every lane of the quad takes part
            if (m < nb) {
                float *dst = wf + (size_t)m * 1024 + (tid >> 2);
#pragma unroll
                for (int k2 = 0; k2 < 16; k2++) {
                    const cf x = u[rev16(k2)] * (1.0f / 4096.0f);
                    const float pw = quad_sum(x.x * x.x + x.y * x.y);
                    if ((tid & 3) == 0) dst[64 * (k2 ^ 8)] = pw;
                }
            }
        }
    }
    __syncthreads();
    // ---- the rows of this wave ---------------------------------------------------------------------------------------------------------
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const unsigned cls = (wcls >> (4 * wave)) & 0xfu;
    const F4Row *wr = srows + 8 * wave;
    F4Row r0{}, r1{};
    RowAt a0{}, a1{};
    if (cls == 1 || cls == 2) {
        const int b = lane & 15;
        r0 = wr[lane >> 4];
        a0 = row_at(r0, 256, m0, nb, mbase, fbm, R, wins, nb_call, tiles);
        {
            cf w[16];
#pragma unroll
            for (int a = 0; a < 16; a++) w[a] = ld2(a0.win + 16 * a + b);
#pragma unroll
            for (int a = 0; a < 16; a++) v[a ^ 8] = cmul(ld2(a0.spec + 16 * a + b), w[a]);      // ifftshift of the slice: i -> i + l/2
        }
        if (cls == 2) {
            r1 = wr[4 + (lane >> 4)];
            a1 = row_at(r1, 256, m0, nb, mbase, fbm, R, wins, nb_call, tiles);
            cf w[16];
#pragma unroll
            for (int a = 0; a < 16; a++) w[a] = ld2(a1.win + 16 * a + b);
#pragma unroll
            for (int a = 0; a < 16; a++) v[16 + (a ^ 8)] = cmul(ld2(a1.spec + 16 * a + b), w[a]);
        }
        dft16<true>(reinterpret_cast<cf (&)[16]>(v[0]));
        if (cls == 2) dft16<true>(reinterpret_cast<cf (&)[16]>(v[16]));
    }
    if constexpr (WIDE) {
        if (cls == 3 || cls == 4) {
            const int L = cls == 3 ? 512 : 1024, lg = cls == 3 ? 4 : 5;
            const int b = lane & ((1 << lg) - 1);
            r0 = wr[lane >> lg];
            a0 = row_at(r0, L, m0, nb, mbase, fbm, R, wins, nb_call, tiles);
            cf w[32];
#pragma unroll
            for (int a = 0; a < 32; a++) w[a] = ld2(a0.win + (a << lg) + b);
#pragma unroll
            for (int a = 0; a < 32; a++) v[a ^ 16] = cmul(ld2(a0.spec + (a << lg) + b), w[a]);
            dft32<true>(v);                                          // over a: index p in v[pos32(p)]
        }
    }
    if (cls >= 5) {
        // l = 128 (8 lanes x 16 points per row), 64 (4 lanes), 32 (2 lanes), 16 (one lane): eight rows on the first 8 * lanes lanes of the wave; slice (a << lg) + b
        const int lg = 8 - (int)cls, b = lane & ((1 << lg) - 1);
        r0 = wr[(lane >> lg) & 7];
        a0 = row_at(r0, 16 << lg, m0, nb, mbase, fbm, R, wins, nb_call, tiles);
        if ((lane >> lg) >= 8) a0.on = false;
        cf w[16];
#pragma unroll
        for (int a = 0; a < 16; a++) w[a] = ld2(a0.win + (a << lg) + b);
#pragma unroll
        for (int a = 0; a < 16; a++) v[a ^ 8] = cmul(ld2(a0.spec + (a << lg) + b), w[a]);          // ifftshift of the slice: i -> i + l/2 = a -> a ^ 8
        dft16<true>(reinterpret_cast<cf (&)[16]>(v[0]));             // over a: index p in v[rev16(p)]
    }
    __syncthreads();                                                 // every slice has been read: the tiles belong to the rows' exchanges
    if (cls == 1 || cls == 2) {
        const int b = lane & 15;
        cf w[16];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float4 t = ld4(&t256[b * 18 + 2 * i]);
            w[2 * i] = mk(t.x, t.y); w[2 * i + 1] = mk(t.z, t.w);
        }
        // element (b, p) of a row at p * 16 + (b ^ p): stores of one p and loads of one b are conflict-free (k_c256)
        float2 *row0 = tiles + r0.xch, *row1 = tiles + r1.xch;
        if (a0.on) {
#pragma unroll
            for (int p = 0; p < 16; p++) st2(&row0[p * 16 + (b ^ p)], cmulc(v[rev16(p)], w[p]));
        }
        if (cls == 2 && a1.on) {
#pragma unroll
            for (int p = 0; p < 16; p++) st2(&row1[p * 16 + (b ^ p)], cmulc(v[16 + rev16(p)], w[p]));
        }
        wave_sync();
#pragma unroll
        for (int bb = 0; bb < 16; bb++) v[bb] = ld2(&row0[b * 16 + (bb ^ b)]);
        if (cls == 2) {
#pragma unroll
            for (int bb = 0; bb < 16; bb++) v[16 + bb] = ld2(&row1[b * 16 + (bb ^ b)]);
        }
        dft16<true>(reinterpret_cast<cf (&)[16]>(v[0]));
        if (cls == 2) dft16<true>(reinterpret_cast<cf (&)[16]>(v[16]));
        // y[t], t = b + 16 q; keep t >= l/R (vector_cut_vxx(l, l - lout, lout)), times l (multiply_const_cc)
        const int skip = 256 - r0.lout;
        if constexpr (FINE) {
            fine_row(fa, 8 * wave + (lane >> 4), r0, m0, 256, fb0, fs0);
            if (cls == 2) fine_row(fa, 8 * wave + 4 + (lane >> 4), r1, m0, 256, fb1, fs1);
        }
        if (a0.on) {
#pragma unroll
            for (int q = 0; q < 16; q++) if (b + 16 * q >= skip) F4_PUT(a0, b + 16 * q, v[rev16(q)] * 256.f, fb0, fs0);
        }
        if (cls == 2 && a1.on) {
#pragma unroll
            for (int q = 0; q < 16; q++) if (b + 16 * q >= skip) F4_PUT(a1, b + 16 * q, v[16 + rev16(q)] * 256.f, fb1, fs1);
        }
    }
    if constexpr (WIDE) {
        // the inter-layer twiddles of both wide forms from ONE table: W_1024^(x p) = W_1024^((x & 15) p) W_64^((x >> 4) p), x < 32;
        // l = 1024: x = b; l = 512: W_512^(b p) = W_1024^(2 b p), x = 2 b
        if (cls == 3 || cls == 4) {
            const int lg = cls == 3 ? 4 : 5, b = lane & ((1 << lg) - 1), x = cls == 3 ? 2 * b : b;
            const float2 *wa = reinterpret_cast<const float2 *>(fdc_smem_f4 + f4_off_w1k(TEAMS)) + (x & 15) * 34;
            const float2 *wb = reinterpret_cast<const float2 *>(fdc_smem_f4 + f4_off_w64(TEAMS)) + (x >> 4) * 34;
            float2 *row = tiles + r0.xch;
            // element (b, p) of a row at p * lanes + (b ^ (p mod lanes)) (k_c1024, k_c512)
            if (a0.on) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const float4 t = ld4(&wa[2 * i]), c = ld4(&wb[2 * i]);
                    st2(&row[((2 * i) << lg) + (b ^ ((2 * i) & ((1 << lg) - 1)))], cmulc(v[pos32(2 * i)], cmul(mk(t.x, t.y), mk(c.x, c.y))));
                    st2(&row[((2 * i + 1) << lg) + (b ^ ((2 * i + 1) & ((1 << lg) - 1)))], cmulc(v[pos32(2 * i + 1)], cmul(mk(t.z, t.w), mk(c.z, c.w))));
                }
            }
            wave_sync();
            if constexpr (FINE) fine_row(fa, 8 * wave + (lane >> lg), r0, m0, 16 << (lg + 1), fb0, fs0);
            if (cls == 4) {
#pragma unroll
                for (int bb = 0; bb < 32; bb++) v[bb] = ld2(&row[b * 32 + (bb ^ b)]);
                dft32<true>(v);                                      // y[t = b + 32 q] in v[pos32(q)]
                const int skip = 1024 - r0.lout;
                if (a0.on) {
#pragma unroll
                    for (int q = 0; q < 32; q++) if (b + 32 * q >= skip) F4_PUT(a0, b + 32 * q, v[pos32(q)] * 1024.f, fb0, fs0);
                }
            } else {
                // l = 512 = 32 x 16: DFT-16 over b for p = lane and p = lane + 16; y[t = p + 32 q]
#pragma unroll
                for (int bb = 0; bb < 16; bb++) {
                    v[bb] = ld2(&row[b * 16 + (bb ^ b)]);
                    v[16 + bb] = ld2(&row[(b + 16) * 16 + (bb ^ b)]);
                }
                dft16<true>(reinterpret_cast<cf (&)[16]>(v[0]));
                dft16<true>(reinterpret_cast<cf (&)[16]>(v[16]));
                const int skip = 512 - r0.lout;
                if (a0.on) {
#pragma unroll
                    for (int q = 0; q < 16; q++) {
                        const int t0 = b + 32 * q, t1 = t0 + 16;
                        if (t0 >= skip) F4_PUT(a0, t0, v[rev16(q)] * 512.f, fb0, fs0);
                        if (t1 >= skip) F4_PUT(a0, t1, v[16 + rev16(q)] * 512.f, fb0, fs0);
                    }
                }
            }
        }
    }
    if (cls >= 5) {
        // y[t = p + 16 q] = sum_b W_l^(-b p) W_(l/16)^(-b q) (DFT-16 over a)[p]: twiddle W_l^(b p) = W_256^((256 / l) b p) from the 256 table, an exchange inside the
        // row — element (b, p) at p * lanes + (b ^ (p mod lanes)) — then every lane runs the DFT-(l/16) over b for its 16 / lanes values of p
        const int lg = 8 - (int)cls, lanes = 1 << lg, b = lane & (lanes - 1);
        cf w[16];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float4 t = ld4(&t256[(b << (4 - lg)) * 18 + 2 * i]);
            w[2 * i] = mk(t.x, t.y); w[2 * i + 1] = mk(t.z, t.w);
        }
        float2 *row = tiles + r0.xch;
        if (a0.on) {
#pragma unroll
            for (int p = 0; p < 16; p++) st2(&row[(p << lg) + (b ^ (p & (lanes - 1)))], cmulc(v[rev16(p)], w[p]));
        }
        wave_sync();
        if constexpr (FINE) fine_row(fa, 8 * wave + ((lane >> lg) & 7), r0, m0, 16 << lg, fb0, fs0);
        if (cls == 5) {
            // p = b and p = b + 8: two DFT-8 (dft8 leaves X[k0 + 2 k1] in [4 k0 + k1])
#pragma unroll
            for (int bb = 0; bb < 8; bb++) {
                v[bb] = ld2(&row[(b << 3) + (bb ^ b)]);
                v[8 + bb] = ld2(&row[((b + 8) << 3) + (bb ^ b)]);
            }
            dft8<true>(reinterpret_cast<cf (&)[8]>(v[0]));
            dft8<true>(reinterpret_cast<cf (&)[8]>(v[8]));
            const int skip = 128 - r0.lout;
            if (a0.on) {
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const int t0 = b + 16 * q, t1 = t0 + 8;
                    if (t0 >= skip) F4_PUT(a0, t0, v[4 * (q & 1) + (q >> 1)] * 128.f, fb0, fs0);
                    if (t1 >= skip) F4_PUT(a0, t1, v[8 + 4 * (q & 1) + (q >> 1)] * 128.f, fb0, fs0);
                }
            }
        } else if (cls == 7) {
            // l = 32: p = b + 2 j, j < 8: eight DFT-2; y[t = p + 16 q], q < 2
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const cf e = ld2(&row[((b + 2 * j) << 1) + b]), o = ld2(&row[((b + 2 * j) << 1) + (1 ^ b)]);
                v[2 * j] = e + o; v[2 * j + 1] = e - o;
            }
            const int skip = 32 - r0.lout;
            if (a0.on) {
#pragma unroll
                for (int j = 0; j < 8; j++) {
#pragma unroll
                    for (int q = 0; q < 2; q++) if (b + 2 * j + 16 * q >= skip) F4_PUT(a0, b + 2 * j + 16 * q, v[2 * j + q] * 32.f, fb0, fs0);
                }
            }
        } else if (cls == 8) {
            // l = 16: the DFT-16 over a is the whole transform (the trip through the row's exchange area only puts y[p] into register p)
#pragma unroll
            for (int p = 0; p < 16; p++) v[p] = ld2(&row[p]);
            const int skip = 16 - r0.lout;
            if (a0.on) {
#pragma unroll
                for (int p = 0; p < 16; p++) if (p >= skip) F4_PUT(a0, p, v[p] * 16.f, fb0, fs0);
            }
        } else {
            // p = b + 4 j, j < 4: four DFT-4
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int bb = 0; bb < 4; bb++) v[4 * j + bb] = ld2(&row[((b + 4 * j) << 2) + (bb ^ b)]);
                dft4<true>(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
            }
            const int skip = 64 - r0.lout;
            if (a0.on) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
#pragma unroll
                    for (int q = 0; q < 4; q++) if (b + 4 * j + 16 * q >= skip) F4_PUT(a0, b + 4 * j + 16 * q, v[4 * j + q] * 64.f, fb0, fs0);
                }
            }
        }
    }
#undef F4_PUT
