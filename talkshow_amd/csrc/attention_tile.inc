// The body of face.hip's attention kernels from the Q fragments to the store, included once per kernel (the uniform kernel, the mixed-pass
// variant and the packed-row variant: one text, three compilations — no kernel's code depends on another's existence).  Expects in scope:
//   base   qkv + the clip's first row + the head's 64 channels          ld     row pitch of qkv (3 HID)
//   T      keys and queries of this clip                                 Tp     clip stride of `out` in rows: clip b starts at row b Tp (0 where `out` already points at the clip's first row)
//   q0     this wave's first query                                       b, h, HID, scale, out, Ks, Vs, tid, wave, li, lg
    // soft-max in base 2: exp(s * scale - max) = 2^(s * scale * log2 e - max'), one v_exp_f32 per probability instead of expf's
    // range reduction (32 of them per lane and key tile: as many VALU slots as the tile's MFMAs have issue slots)
    const float scale2 = scale * 1.44269504088896341f;
    // Q fragments (pre-multiplied by scale * log2 e), B operand of the first product: lane (li, lg) holds Q[q0 + li][16 qs + 4 lg + e]; rows past T are clamped (computed, never stored)
    f32x4 qf[4];
    {
        const int qrow = q0 + li < T ? q0 + li : T - 1;
#pragma unroll
        for (int qs = 0; qs < 4; ++qs) qf[qs] = *reinterpret_cast<const f32x4 *>(base + (long)qrow * ld + 16 * qs + 4 * lg) * scale2;
    }
    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const bool live = q0 < T;   // wave-uniform: this wave has at least one real query (it still stages K / V and meets the barriers)
    for (int k0 = 0; k0 < T; k0 += 64) {
        __syncthreads();   // every wave is done reading the previous tile
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 4) + 16 * i, col = (tid & 15) * 4, key = k0 + row;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (key < T) {
                kv = *reinterpret_cast<const f32x4 *>(base + (long)key * ld + HID + col);
                vv = *reinterpret_cast<const f32x4 *>(base + (long)key * ld + 2 * HID + col);
            }
            *reinterpret_cast<f32x4 *>(&Ks[row * ATT_P + col]) = kv;
            *reinterpret_cast<f32x4 *>(&Vs[row * ATT_P + col]) = vv;
        }
        __syncthreads();
        // The products of one key tile for NKB real 16-key blocks (compile-time: the MFMA stream has no branches in it).  The key block /
        // d block is the INNER loop of both products: four independent accumulators take turns, so an MFMA never waits for its
        // predecessor's result (16 in a row on one accumulator issue every 40 cycles, not 32).  Key blocks wholly beyond T (the last
        // tile of a 300-frame clip has three real blocks) are not multiplied, nor are waves whose 16 queries all lie beyond T.
        auto tile = [&](auto NKBc, auto RAGc) {
            constexpr int NKB = decltype(NKBc)::value;
            constexpr bool RAGGED = decltype(RAGc)::value != 0;   // the tile reaches beyond T: its padding keys are masked
            f32x4 sacc[NKB];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) sacc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int qs = 0; qs < 4; ++qs) {
                f32x4 kf[NKB];
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) kf[kb] = *reinterpret_cast<const f32x4 *>(&Ks[(kb * 16 + li) * ATT_P + 16 * qs + 4 * lg]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int kb = 0; kb < NKB; ++kb) sacc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][e], qf[qs][e], sacc[kb], 0, 0, 0);
            }
            // scale, mask the padding keys, online soft-max of query li (this lane's keys: k0 + 16 kb + 4 lg + r)
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (RAGGED && (k0 + kb * 16 + 4 * lg + r) >= T) sacc[kb][r] = -INFINITY;
                    mx = fmaxf(mx, sacc[kb][r]);
                }
            mx = rows_allreduce(mx, [](float a, float b) { return fmaxf(a, b); });
            const float m_new = fmaxf(m, mx);          // finite: every tile holds at least one real key
            const float alpha = __builtin_amdgcn_exp2f(m - m_new);       // first tile: 2^-inf = 0
            float rs = 0.f;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(sacc[kb][r] - m_new);
                    sacc[kb][r] = pv;
                    rs += pv;
                }
            rs = rows_allreduce(rs, [](float a, float b) { return a + b; });
            l = l * alpha + rs;
            m = m_new;
#pragma unroll
            for (int db = 0; db < 4; ++db) o[db] *= alpha;
            // O^T += V^T P^T; the B operand is the probability registers as they are.  The A operand V^T[d = li][key = 4 lg + e] is read
            // from V as it was staged ([key][d], 16 consecutive d per lane group: four ds_read_b32, rows 4 lg + e of a 68-float pitch
            // land 16 banks apart for lg and lg + 1: conflict-free) — a transposed copy of V would need 16 scattered ds_write_b32 per
            // thread and tile, 8 lanes to a bank (measured: 63 % of the LDS cycles were conflicts)
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float va[4];
#pragma unroll
                    for (int db = 0; db < 4; ++db) va[db] = Vs[(kb * 16 + 4 * lg + e) * ATT_P + db * 16 + li];
#pragma unroll
                    for (int db = 0; db < 4; ++db) o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[db], sacc[kb][e], o[db], 0, 0, 0);
                }
        };
        if (live) {
            const int nkb = (T - k0 + 15) >> 4;
            if (k0 + 64 <= T) tile(IC4<4>{}, IC4<0>{});
            else if (nkb >= 4) tile(IC4<4>{}, IC4<1>{});
            else if (nkb == 3) tile(IC4<3>{}, IC4<1>{});
            else if (nkb == 2) tile(IC4<2>{}, IC4<1>{});
            else tile(IC4<1>{}, IC4<1>{});
        }
    }
    if (q0 + li < T) {
        const float inv = 1.0f / l;
        float *dst = out + ((long)b * Tp + q0 + li) * HID + h * 64 + 4 * lg;
#pragma unroll
        for (int db = 0; db < 4; ++db) *reinterpret_cast<f32x4 *>(dst + db * 16) = o[db] * inv;
    }
