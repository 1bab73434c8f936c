// bevw_body_stitch_pp.h -- the body of k_stitch_pp and k_stitch_pp_yuv422 (bevw_kernels.h).
// Included inside a kernel's braces, NOT a device function: the kernels that existed before the packed 4:2:2 formats stay the functions the
// compiler saw then and compile to the same instructions (the same body inlined from a device function schedules differently).  In scope at
// the point of inclusion: the kernel's parameters, the layout SRC of the frames, the flags BLEND, BAL, OUT_NV12, and `ypos` (the Y byte's position; 4:2:2 only).
    __shared__ HsvTables hsv;
    __shared__ unsigned long long part[3][4];
    if (BAL) {
        hsv_tables_to_lds(hsv, tab);
        __syncthreads();
    }
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int b = blockIdx.z;
    const size_t frame_bytes = Src<SRC>::frame_bytes((size_t)fw * fh);
    int acc[3] = {0, 0, 0};
    if (x < bw) {
        const size_t o = (size_t)y * bw + x;
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
            const int m = T.mask[c][o];
            if (m == 0) continue;
            const uint8_t *src = frames + ((size_t)b * 4 + c) * frame_bytes;
            const int sx = T.lut1[c][o * 2], sy = T.lut1[c][o * 2 + 1];
            int v[3];
            if constexpr (Src<SRC>::surf) {
                const Nv12Surface sf = surf[(size_t)b * 4 + c];
                remap_u8c3_px<BAL, SRC>(sf.y, fw, fh, sx, sy, T.lut2[c][o] & (kQTab2 - 1), v, BAL ? deltas[b * 4 + c] : 0, &hsv, ties_even, sf.uv,
                                               src_pitch);
            } else
            remap_u8c3_px<BAL, SRC>(src, fw, fh, sx, sy, T.lut2[c][o] & (kQTab2 - 1), v, BAL ? deltas[b * 4 + c] : 0, &hsv, ties_even, nullptr, 0, ypos);
            if (BLEND) {
                const float wgt = blend_weight_f32(m);
                v[0] = blend_mul(v[0], wgt); v[1] = blend_mul(v[1], wgt); v[2] = blend_mul(v[2], wgt);
            }
            acc[0] = min(255, acc[0] + v[0]); acc[1] = min(255, acc[1] + v[1]); acc[2] = min(255, acc[2] + v[2]);
        }
        uint8_t *d = out + ((size_t)b * bw * bh + o) * 3;
        if (!BAL && car != nullptr) {
            acc[0] = min(255, acc[0] + car[o * 3]); acc[1] = min(255, acc[1] + car[o * 3 + 1]);
            acc[2] = min(255, acc[2] + car[o * 3 + 2]);
        }
        if (OUT_NV12) {
            static_assert(!(OUT_NV12 && BAL), "balance: the pre-gain image is BGR, the gain pass writes NV12");
            nv12_store_px(out + (size_t)b * image_bytes_of(bw, bh, true), bw, bh, x, y,
                          (uint32_t)acc[0] | ((uint32_t)acc[1] << 8) | ((uint32_t)acc[2] << 16));
        } else {
            d[0] = (uint8_t)acc[0]; d[1] = (uint8_t)acc[1]; d[2] = (uint8_t)acc[2];
        }
    }
    if (BAL) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            unsigned s = wave_sum_u32((unsigned)acc[k]);
            if (lane == 0) part[k][wv] = s;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            unsigned long long t = 0;
            for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += part[threadIdx.x][i];
            atomicAdd(&chsums[b * 3 + threadIdx.x], t);
        }
    }
