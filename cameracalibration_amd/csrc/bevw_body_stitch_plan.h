// bevw_body_stitch_plan.h -- the body of k_stitch_plan and k_stitch_plan_yuv422 (bevw_plan.h).
// Included inside a kernel's braces, NOT a device function: the kernels that existed before the packed 4:2:2 formats stay the functions the
// compiler saw then and compile to the same instructions (the same body inlined from a device function schedules differently).  In scope at
// the point of inclusion: `a` (PlanArgs), the layout SRC of its frames (SrcLayout) and the flags BLEND, LUM, SUMS, OUT_NV12.
    constexpr bool BAL = LUM;
    __shared__ __attribute__((aligned(16))) uint32_t hsv_words[BAL ? sizeof(HsvTables) / 4 : 1];   // (no LDS for the variants without the luminance round trip)
    const HsvTables &hsv = *reinterpret_cast<const HsvTables *>(hsv_words);
    if (BAL) {
        hsv_tables_to_lds(*reinterpret_cast<HsvTables *>(hsv_words), a.tab);
        __syncthreads();
    }
    uint32_t chunk, group;
    if (!plan_block_map(a, blockIdx.x, chunk, group)) return;
    const int lane = threadIdx.x & 63;
    const int slot = (int)group * (int)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (slot >= a.nlist) return;
    const int tile = a.tile_list ? (int)__builtin_amdgcn_readfirstlane(a.tile_list[slot]) : slot;

    const uint32_t hdr = __builtin_amdgcn_readfirstlane(a.hdr[tile]);
    const bool second = hdr & kHdrSecond, tile_slow = hdr & kHdrSlow;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int x0 = (tx * kPlanLX + lane % kPlanLX) * 4, y = ty * kPlanLY + lane / kPlanLX;
    const bool inimg = x0 < a.bw && y < a.bh;
    const uint32_t frame_bytes = (uint32_t)a.fw * a.fh * 3, row_bytes = (uint32_t)a.fw * 3;
    const uint32_t src_frame = Src<SRC>::frame_bytes_of_bgr(frame_bytes);   // bytes of one camera frame as the kernel reads it
    const size_t set_bytes = (size_t)src_frame * a.ncams, img_bytes = (size_t)a.pitch * a.bh * 3;
    const uint32_t ooff = ((uint32_t)y * a.pitch + x0) * 3;

    EntryRegs e0[4], e1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        e0[j] = decode_entry(a.plan[((size_t)tile * 8 + j) * 64 + lane], BLEND);
        e1[j] = decode_entry(second ? a.plan[((size_t)tile * 8 + 4 + j) * 64 + lane] : make_uint2(0, 0), BLEND);
        if (Src<SRC>::yuv) { entry_to_taps(e0[j], a.fw, frame_bytes); entry_to_taps(e1[j], a.fw, frame_bytes); }
    }
    uint32_t car0 = 0, car1 = 0, car2 = 0;
    if (!SUMS && a.car != nullptr && inimg) {
        const uint32_t *cp = reinterpret_cast<const uint32_t *>(a.car + ooff);
        car0 = cp[0]; car1 = cp[1]; car2 = cp[2];
    }
    const bool car_any = __builtin_amdgcn_ballot_w64((car0 | car1 | car2) != 0) != 0;

    const int b_begin = (int)chunk * a.nb, b_end = min(a.batch, b_begin + a.nb);
#pragma unroll 1
    for (int b = b_begin; b < b_end; ++b) {
        const uint8_t *fb = Src<SRC>::surf ? nullptr : a.frames + (size_t)b * set_bytes;
        const Nv12Surface *fs = Src<SRC>::surf ? a.surf + (size_t)b * a.ncams : nullptr;
        const int *fdeltas = BAL ? a.deltas + b * 4 : nullptr;
        int px[4][3];
        if (hdr & kHdrEmpty) {
#pragma unroll
            for (int j = 0; j < 4; ++j) px[j][0] = px[j][1] = px[j][2] = 0;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                eval_entry<BLEND, BAL, SRC>(fb, e0[j], row_bytes, a.fw, a.fh, src_frame, tile_slow, fdeltas, hsv, px[j], fs, a.src_pitch, a.yuv422.ysel & 1u);
            }
            if (second) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int w[3];
                    eval_entry<BLEND, BAL, SRC>(fb, e1[j], row_bytes, a.fw, a.fh, src_frame, tile_slow, fdeltas, hsv, w, fs, a.src_pitch, a.yuv422.ysel & 1u);
                    px[j][0] = min(255, px[j][0] + w[0]); px[j][1] = min(255, px[j][1] + w[1]); px[j][2] = min(255, px[j][2] + w[2]);
                }
            }
        }
        if (SUMS) {
            // per-tile channel sums of the pre-gain BEV (color_balance means, surroundBEV.py:44-47); pixels outside
            // the image have no plan entry and contribute 0.  One entry per listed tile (PlanArgs::sum_base).
            unsigned s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { s0 += px[j][0]; s1 += px[j][1]; s2 += px[j][2]; }
            s0 = wave_sum_u32(s0); s1 = wave_sum_u32(s1); s2 = wave_sum_u32(s2);
            if (lane == 0) {
                uint32_t *ps = a.psums + ((size_t)b * a.nsum + a.sum_base + slot) * 3;
                ps[0] = s0; ps[1] = s1; ps[2] = s2;
            }
        }
        uint32_t P[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) P[j] = (uint32_t)px[j][0] | ((uint32_t)px[j][1] << 8) | ((uint32_t)px[j][2] << 16);
        if (!SUMS && car_any) add_car(P, car0, car1, car2);
        if (OUT_NV12) {
            static_assert(!(OUT_NV12 && SUMS), "balance: the pre-gain image is BGR, the gain pass writes NV12");
            if (inimg) {
                uint32_t yw, uvw;
                nv12_quad(P, yw, uvw);
                uint8_t *img = a.out + (size_t)b * image_bytes_of(a.pitch, a.bh, true);
                *reinterpret_cast<uint32_t *>(img + nv12_y_offset(a.pitch, x0, y)) = yw;
                if (!(y & 1)) *reinterpret_cast<uint32_t *>(img + nv12_uv_offset(a.pitch, a.bh, x0, y)) = uvw;
            }
        } else if (inimg) {
            uint32_t d0, d1, d2;
            pack_pixels(P, d0, d1, d2);
            uint32_t *op = reinterpret_cast<uint32_t *>(a.out + (size_t)b * img_bytes + ooff);
            op[0] = d0; op[1] = d1; op[2] = d2;
        }
    }
