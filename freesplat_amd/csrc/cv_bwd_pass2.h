// Backward pass 2 of the two-pass cost-volume backward: the source-tile sweep (cost_volume.hip, see the comment above its
// #include).  Included twice, inside namespace fs: FS_CV_DET = 0 defines cv_src_grad_kernel (split plane chunks added with
// float atomics), FS_CV_DET = 1 cv_src_grad_det_kernel (chunk c > 0 stores into slab c - 1; cv_det_slab_sum_kernel adds the
// slabs in chunk order).  The default kernel's preprocessed text is exactly the one kernel this file replaced.
template <int C>
__global__ __launch_bounds__(64) void
#if FS_CV_DET
cv_src_grad_det_kernel(
#else
cv_src_grad_kernel(
#endif
    int B, int K, int h, int w, int D, int chunks, int tiles_x, int tiles_y, const float* __restrict__ curT,
    const float4* __restrict__ recS, const float2* __restrict__ recM, const float* __restrict__ Pmat,
    const float* __restrict__ Ginv, const float* __restrict__ cur_invK, const float* __restrict__ planes, long long ps_b,
    long long ps_d, float* __restrict__ d_src
#if FS_CV_DET
    , float* __restrict__ sslab
#endif
    )
{
    constexpr int TW = kSgTW, TH = kSgTH, NT = TW * TH, NV = C / 4, ST = C + 4, G = kSgG;
    static_assert(NT == 64, "one texel per lane");
    __shared__ __attribute__((aligned(16))) float acc[NT * ST];          // the batch's staged records
    __shared__ uint32_t claim_[64];                                      // entries in each texel's list
    __shared__ uint2 lst_[64 * kSgCap];                                  // (pixel lane, weight bits)
    float4 accr[NV];                                                     // this lane's texel
    const int hw = h * w, T = tiles_x * tiles_y;
    // XCD x (= workgroup id % 8) owns the x-th contiguous range of tiles of every view: the workgroups in flight on an XCD
    // -- the same tiles of all K sources, which read the same records -- share one L2
    const int xcd = (int)(blockIdx.x & 7u), jb = (int)(blockIdx.x >> 3);
    const int gb = (T + 7) >> 3, per_b = gb * K * chunks;
    const int b = jb / per_b;
    const int r0 = jb - b * per_b, tl = r0 / (K * chunks), r1 = r0 - tl * (K * chunks);
    const int k = r1 / chunks, chunk = r1 - k * chunks;
    const int tile = xcd * gb + tl;
    if (b >= B || tile >= T) return;   // (workgroup-uniform)
    const int tx0 = (tile % tiles_x) * TW, ty0 = (tile / tiles_x) * TH;
    const int tw_ = min(TW, w - tx0), th_ = min(TH, h - ty0);
    const int lane = threadIdx.x;
    claim_[lane] = 0u;
#pragma unroll
    for (int s = 0; s < NV; ++s) accr[s] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    wave_lds_sync();
    volatile uint32_t* const claim = claim_;
    const float* P = Pmat + ((size_t)b * K + k) * 12;
    const float* iK = cur_invK + (size_t)b * 16;
    const float inv_w = (float)(1.0 / (double)w), inv_h = (float)(1.0 / (double)h);
    const int dchunk = (D + chunks - 1) / chunks;
    const int d0 = min(D, chunk * dchunk), d1 = min(D, d0 + dchunk);
    const float X0 = (float)tx0 - 0.55f, X1 = (float)(tx0 + tw_) + 0.55f;     // qx / qz = ix + 0.5, taps at floor(ix), + 1
    const float Y0 = (float)ty0 - 0.55f, Y1 = (float)(ty0 + th_) + 0.55f;
    const uint32_t kbit = 2u * (uint32_t)k;

    struct Geo { int t00; float tx, ty; uint32_t okm; bool pend; };

    // The four planes of a group lie a quarter of the sweep apart (dg + g * gstride): walked together, the same pixel in
    // two of them samples texels many disparity steps apart -- with neighbouring planes (~0.56 texel apart at the native
    // size) every batch that straddles two planes had lanes with the same tap base, i.e. a second claim round of the round-4 form.
    const int gstride = (d1 - d0 + G - 1) / G;
    for (int dg = d0; dg < d0 + gstride; ++dg) {
        // ---- the tile's preimage boxes in the current view, four planes at once: lane 4 g + q = corner q of its plane ----
        int bx0s[G], by0s[G], Wbs[G], ns[G];
        float rcps[G], deps[G];
        {
            const int g = (lane >> 2) & 3, q = lane & 3, d = dg + g * gstride;
            const float* Gi = Ginv + (((size_t)b * K + k) * D + min(d, D - 1)) * 9;
            const float X = (q & 1) ? X1 : X0, Y = (q & 2) ? Y1 : Y0;
            const float cu = fmaf(Gi[0], X, fmaf(Gi[1], Y, Gi[2]));
            const float cv_ = fmaf(Gi[3], X, fmaf(Gi[4], Y, Gi[5]));
            const float cc = fmaf(Gi[6], X, fmaf(Gi[7], Y, Gi[8]));
            auto qx1 = [](float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)); };   // lane ^ 1
            auto qx2 = [](float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true)); };   // lane ^ 2
            auto qmin = [&](float v) { v = fminf(v, qx1(v)); return fminf(v, qx2(v)); };
            auto qmax = [&](float v) { v = fmaxf(v, qx1(v)); return fmaxf(v, qx2(v)); };
            float csum = cc + qx1(cc);
            csum += qx2(csum);
            const float cmin = qmin(cc), cmax = qmax(cc);
            const float amax = fmaxf(fabsf(cmin), fabsf(cmax));
            const bool finite = csum * 0.0f == 0.0f;                               // (NaN / inf in the inverse: whole image)
            const bool behind = finite && cmax < -1e-3f * amax;                    // tile entirely behind the source: z_k < 0
            const bool front = finite && cmin > 1e-3f * amax;
            const float u = cu / cc - 0.5f, v = cv_ / cc - 0.5f;
            const float umin = qmin(u), umax = qmax(u), vmin = qmin(v), vmax = qmax(v);
            int bx0 = 0, bx1 = w - 1, by0 = 0, by1 = h - 1;
            const bool boxed = front && (umin + umax + vmin + vmax) * 0.0f == 0.0f;
            if (boxed) {
                bx0 = (int)fminf(fmaxf(ceilf(umin - 0.05f), 0.0f), (float)w);
                bx1 = (int)fmaxf(fminf(floorf(umax + 0.05f), (float)(w - 1)), -1.0f);
                by0 = (int)fminf(fmaxf(ceilf(vmin - 0.05f), 0.0f), (float)h);
                by1 = (int)fmaxf(fminf(floorf(vmax + 0.05f), (float)(h - 1)), -1.0f);
            }
            int Wb = max(0, bx1 - bx0 + 1), Hb = max(0, by1 - by0 + 1);
            if (behind || d >= d1) Wb = 0;
            const int n = Wb * Hb;
            const float rcp = 1.0f / (float)max(Wb, 1);
            const float dep = planes[b * ps_b + (long long)min(d, D - 1) * ps_d];
#ifdef FS_CV_SG_STATS
            if (lane < 16 && q == 0 && d < d1) {
                if (behind) FS_SG_COUNT(4, 1); else if (n > 0) { FS_SG_COUNT(2, 1); FS_SG_COUNT(5, n); if (!boxed) FS_SG_COUNT(3, 1); }
            }
#endif
#pragma unroll
            for (int gg = 0; gg < G; ++gg) {
                bx0s[gg] = __builtin_amdgcn_readlane(bx0, 4 * gg);
                by0s[gg] = __builtin_amdgcn_readlane(by0, 4 * gg);
                Wbs[gg] = __builtin_amdgcn_readlane(Wb, 4 * gg);
                ns[gg] = __builtin_amdgcn_readlane(n, 4 * gg);
                rcps[gg] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rcp), 4 * gg));
                deps[gg] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dep), 4 * gg));
            }
        }
        const int o1 = ns[0], o2 = o1 + ns[1], o3 = o2 + ns[2], N = o3 + ns[3];
        if (N == 0) continue;

        // ---- one batch of 64 pixels: geometry (the first pass's projection, op by op: warp_source), record loads ----
        auto stage = [&](int i0, Geo& ge, float4 (&S)[NV]) __attribute__((always_inline)) {
            const int i = i0 + lane;
            const bool act = i < N;
            const int gs = (i >= o1 ? 1 : 0) + (i >= o2 ? 1 : 0) + (i >= o3 ? 1 : 0);
            auto sel = [&](auto a0, auto a1, auto a2, auto a3) { return gs == 0 ? a0 : (gs == 1 ? a1 : (gs == 2 ? a2 : a3)); };
            const int loc = i - sel(0, o1, o2, o3);
            const int Wb = sel(Wbs[0], Wbs[1], Wbs[2], Wbs[3]);
            const float rcpW = sel(rcps[0], rcps[1], rcps[2], rcps[3]);
            const float depth = sel(deps[0], deps[1], deps[2], deps[3]);
            int row = (int)(((float)loc + 0.5f) * rcpW), col = loc - row * Wb;
            if (col < 0) { --row; col += Wb; } else if (col >= Wb) { ++row; col -= Wb; }
            const int pu = act ? sel(bx0s[0], bx0s[1], bx0s[2], bx0s[3]) + col : 0;
            const int pv = act ? sel(by0s[0], by0s[1], by0s[2], by0s[3]) + row : 0;
            const int pix = pv * w + pu;
            const float ux = (float)pu + 0.5f, vy = (float)pv + 0.5f;
            const float rx = iK[0] * ux + iK[1] * vy + iK[2];
            const float ry = iK[4] * ux + iK[5] * vy + iK[6];
            const float rz = iK[8] * ux + iK[9] * vy + iK[10];
            const float Xw = depth * rx, Yw = depth * ry, Zw = depth * rz;
            const float qx = P[0] * Xw + P[1] * Yw + P[2] * Zw + P[3];
            const float qy = P[4] * Xw + P[5] * Yw + P[6] * Zw + P[7];
            const float qz = P[8] * Xw + P[9] * Yw + P[10] * Zw + P[11];
            const float zz = qz + 1e-8f;
            const float sc = (fabsf(qz) > 1e-8f) ? 1.0f / zz : 1.0f;
            const float uvx = __fsub_rn(__fmul_rn(__fmul_rn(2.0f, __fmul_rn(qx, sc)), inv_w), 1.0f);
            const float uvy = __fsub_rn(__fmul_rn(__fmul_rn(2.0f, __fmul_rn(qy, sc)), inv_h), 1.0f);
            const float ix = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(uvx, 1.0f), (float)w), 1.0f), 0.5f);
            const float iy = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(uvy, 1.0f), (float)h), 1.0f), 0.5f);
            const float fx0 = floorf(ix), fy0 = floorf(iy);
            ge.tx = ix - fx0; ge.ty = iy - fy0;
            // tap (ox, oy) = texel (fx0 + ox, fy0 + oy): inside the source image AND inside this tile
            const float lx = fx0 - (float)tx0, ly = fy0 - (float)ty0;
            const bool okx0 = lx >= 0.0f && lx <= (float)(tw_ - 1), okx1 = lx >= -1.0f && lx <= (float)(tw_ - 2);
            const bool oky0 = ly >= 0.0f && ly <= (float)(th_ - 1), oky1 = ly >= -1.0f && ly <= (float)(th_ - 2);
            ge.okm = (okx0 && oky0 ? 1u : 0u) | (okx1 && oky0 ? 2u : 0u) | (okx0 && oky1 ? 4u : 0u) | (okx1 && oky1 ? 8u : 0u);
            bool pend = act && zz > 0.0f && ge.okm != 0u;
            ge.t00 = pend ? (int)ly * TW + (int)lx : 0;       // tile-local index of tap (0, 0), >= -(TW + 1)
            if (pend) {
                const size_t pl = (size_t)b * D + (size_t)(dg + gs * gstride);
                const float2 mt = recM[pl * hw + pix];
                const uint32_t fl = __float_as_uint(mt.y) >> kbit;
                pend = (fl & 2u) != 0u;                       // (the first pass's own z_k > 0)
                const float4* sp = recS + (pl * hw + pix) * NV;
#pragma unroll
                for (int s = 0; s < NV; ++s) S[s] = sp[s];
                if (pend && !(fl & 1u)) {
                    // in front, not averaged (an exactly zero score): only d dot / cnt * cur reaches this source
                    const float4* c4 = (const float4*)(curT + ((size_t)b * hw + pix) * C);
#pragma unroll
                    for (int s = 0; s < NV; ++s) {
                        const float4 cv4 = c4[s];
                        S[s] = make_float4(mt.x * cv4.x, mt.x * cv4.y, mt.x * cv4.z, mt.x * cv4.w);
                    }
                }
            }
            ge.pend = pend;
#ifdef FS_CV_SG_STATS
            {
                const unsigned long long hit = __builtin_amdgcn_ballot_w64(pend);
                if (lane == 0) { FS_SG_COUNT(0, 1); FS_SG_COUNT(1, __builtin_popcountll(hit)); }
            }
#endif
        };
        // ---- records to the staging rows, taps to their texels' lists; then every texel lane blends its list ----
        struct Taps { int t00; float tx, ty; uint32_t todo; };
        auto place_taps = [&](Taps& tp) __attribute__((always_inline)) {
#pragma unroll
            for (int tap = 0; tap < 4; ++tap) {
                const int ox = tap & 1, oy = tap >> 1;
                if (tp.todo & (1u << tap)) {
                    const int tt = tp.t00 + oy * TW + ox;
                    const uint32_t slot = atomicAdd(&claim_[tt], 1u);
                    if (slot < (uint32_t)kSgCap) {
                        const float wt = (ox ? tp.tx : 1.0f - tp.tx) * (oy ? tp.ty : 1.0f - tp.ty);
                        lst_[tt * kSgCap + slot] = make_uint2((uint32_t)lane, __float_as_uint(wt));
                        tp.todo &= ~(1u << tap);
                    }
                }
            }
        };
        auto put_records = [&](const Geo& ge, const float4 (&S)[NV]) __attribute__((always_inline)) -> Taps {
            if (ge.pend) {
#pragma unroll
                for (int s = 0; s < NV; ++s) ((float4*)(acc + lane * ST))[s] = S[s];
            }
            Taps tp{ge.t00, ge.tx, ge.ty, ge.pend ? ge.okm : 0u};
            place_taps(tp);
            return tp;
        };
        auto blend_lists = [&](Taps tp) __attribute__((always_inline)) {
            for (;;) {
                wave_lds_sync();
                const int nl = (int)min(claim[lane], (uint32_t)kSgCap);
#pragma unroll 1
                for (int e = 0; e < kSgCap; ++e) {
                    if (__builtin_amdgcn_ballot_w64(e < nl) == 0ull) break;
                    if (e < nl) {
                        const uint2 en = lst_[lane * kSgCap + e];
                        const float wt = __uint_as_float(en.y);
                        const float4* sp = (const float4*)(acc + en.x * ST);
#pragma unroll
                        for (int s = 0; s < NV; ++s) {
                            const float4 v = sp[s];
                            accr[s].x = fmaf(wt, v.x, accr[s].x); accr[s].y = fmaf(wt, v.y, accr[s].y);
                            accr[s].z = fmaf(wt, v.z, accr[s].z); accr[s].w = fmaf(wt, v.w, accr[s].w);
                        }
                    }
                }
                claim[lane] = 0u;
                wave_lds_sync();
                if (__builtin_amdgcn_ballot_w64(tp.todo != 0u) == 0ull) break;
                place_taps(tp);          // (taps that found their texel's list full: the staged records are still there)
            }
        };
        // one record buffer: the next batch's loads are issued as soon as this batch's records sit in their staging rows, and
        // are in flight while the lists are blended (a second register buffer costs the third wavefront per SIMD: 3.0 vs 2.8 ms)
        Geo gA;
        float4 SA[NV];
        stage(0, gA, SA);
        for (int i0 = 0; i0 < N; i0 += 64) {
            const Taps tp = put_records(gA, SA);
            if (i0 + 64 < N) stage(i0 + 64, gA, SA);
            blend_lists(tp);
        }
    }
    wave_lds_sync();
    // ---- the tile leaves once, in the caller's [C, h, w] layout ----
    {
#if FS_CV_DET
        // (plane chunk c > 0: its own slab, added in chunk order by cv_det_slab_sum_kernel)
        float* const dmap = (chunk > 0 ? sslab + (size_t)(chunk - 1) * B * K * C * hw : d_src) + (((size_t)b * K + k) * C) * hw;
#else
        float* const dmap = d_src + (((size_t)b * K + k) * C) * hw;
#endif
        const int ty = lane / TW, tx = lane % TW;
        const bool inside = lane < NT && tx < tw_ && ty < th_;
        float* const dpx = dmap + (size_t)(ty0 + ty) * w + (tx0 + tx);
#pragma unroll
        for (int s = 0; s < NV; ++s) {
            const float4 v = accr[s];
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ch = 4 * s + e;
#if FS_CV_DET
                if (inside) dpx[(size_t)ch * hw] = vv[e];
#else
                if (inside) { if (chunks > 1) atomicAdd(dpx + (size_t)ch * hw, vv[e]); else dpx[(size_t)ch * hw] = vv[e]; }
#endif
            }
        }
    }
}
