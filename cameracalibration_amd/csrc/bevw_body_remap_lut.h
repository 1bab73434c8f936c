// bevw_body_remap_lut.h -- the body of k_remap_lut and k_remap_lut_yuv422 (bevw_kernels.h).
// Included inside a kernel's braces, NOT a device function: the kernels that existed before the packed 4:2:2 formats stay the functions the
// compiler saw then and compile to the same instructions (the same body inlined from a device function schedules differently).  In scope at
// the point of inclusion: the kernel's parameters, the layout SRC of the sources, the flag OUT_NV12, and `ypos` (the Y byte's position; 4:2:2 only).
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= dw) return;
    const size_t o = (size_t)y * dw + x;
    const uint8_t *s = src + (size_t)blockIdx.z * Src<SRC>::frame_bytes((size_t)sw * sh);
    const int sx = map1[o * 2], sy = map1[o * 2 + 1];
    int out[3];
    if constexpr (Src<SRC>::surf) {
        const Nv12Surface sf = surf[blockIdx.z];
        remap_u8c3_px<false, SRC>(sf.y, sw, sh, sx, sy, map2[o] & (kQTab2 - 1), out, 0, nullptr, ties_even, sf.uv, src_pitch);
    } else {
        remap_u8c3_px<false, SRC>(s, sw, sh, sx, sy, map2[o] & (kQTab2 - 1), out, 0, nullptr, ties_even, nullptr, 0, ypos);
    }
    if (OUT_NV12) {
        nv12_store_px(dst + (size_t)blockIdx.z * image_bytes_of(dw, dh, true), dw, dh, x, y,
                      (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16));
        return;
    }
    uint8_t *d = dst + ((size_t)blockIdx.z * dw * dh + o) * 3;
    d[0] = (uint8_t)out[0]; d[1] = (uint8_t)out[1]; d[2] = (uint8_t)out[2];
