// bevw_body_lum_groups.h -- the body of k_lum_groups and k_lum_groups_yuv422 (bevw_plan.h).
// Included inside a kernel's braces, NOT a device function: the kernels that existed before the packed 4:2:2 formats stay the functions the
// compiler saw then and compile to the same instructions (the same body inlined from a device function schedules differently).  In scope at
// the point of inclusion: the kernel's parameters, the layout SRC of the raw frames (SrcLayout), and `order` (Yuv422Order; packed 4:2:2 only).
    __shared__ HsvTables hsv;
    __shared__ int cam_delta[4];
    uint32_t frame, blk;
    if (!xcd_frame_map(blockIdx.x, blocks_per_frame, nframes, frame, blk)) return;   // grid: xcd_frame_grid()
    hsv_tables_to_lds(hsv, tab);
    if (threadIdx.x < 4) cam_delta[threadIdx.x] = deltas[frame * 4 + threadIdx.x];   // k_lum_delta's (a kernel of its own: bevwarp.hip luminance_stats)
    const uint8_t *fin = frames + (size_t)frame * set_bytes;
    uint8_t *fout = scratch + (size_t)frame * scratch_stride;
    const int g0 = (int)blk * (kLumTrips * 256) + (int)threadIdx.x;
    uint32_t goff[kLumTrips], coff[kLumTrips];
    AlignedU3 v[kLumTrips];
    if (Src<SRC>::nv12) {
#pragma unroll
        for (int t = 0; t < kLumTrips; ++t) {
            const bool in = g0 + t * 256 < ngroups;
            goff[t] = in ? groups[2 * (g0 + t * 256)] : 0u;
            coff[t] = in ? groups[2 * (g0 + t * 256) + 1] : 0u;
        }
#pragma unroll
        for (int t = 0; t < kLumTrips; ++t) {   // v.x = Y bytes, v.y = U / V bytes of texels x .. x+3
            if constexpr (Src<SRC>::surf) {   // (past the list: texels 0 .. 3 of camera 0 once more, not stored)
                const Nv12Surface sf = surf[(size_t)frame * 4 + unit_surf_cam(coff[t])];
                v[t].x = *reinterpret_cast<const uint32_t *>(sf.y + goff[t]);
                v[t].y = *reinterpret_cast<const uint32_t *>(sf.uv + unit_surf_uv(coff[t]));
            } else {
                v[t].x = *reinterpret_cast<const uint32_t *>(fin + goff[t]);
                v[t].y = *reinterpret_cast<const uint32_t *>(fin + coff[t]);
            }
            v[t].z = 0u;
        }
    } else {
#pragma unroll
        for (int t = 0; t < kLumTrips; ++t) goff[t] = g0 + t * 256 < ngroups ? groups[g0 + t * 256] : 0u;
#pragma unroll
        for (int t = 0; t < kLumTrips; ++t) {
            if (Src<SRC>::p422) {   // v.x = Y bytes, v.y = U / V bytes of texels x .. x+3, as on the NV12 path
                const uint2 w = *reinterpret_cast<const uint2 *>(fin + goff[t]);
                yuv422_split(w.x, w.y, order, v[t].x, v[t].y);
                v[t].z = 0u;
            } else
            v[t] = *reinterpret_cast<const AlignedU3 *>(fin + goff[t]);   // (past the list: group 0 once more, not stored)
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kLumTrips; ++t) {
        const int gi = g0 + t * 256;
        if (gi >= ngroups) break;
        const uint32_t w[3] = {v[t].x, v[t].y, v[t].z};
        const int cam = Src<SRC>::surf ? (int)unit_surf_cam(coff[t]) : (int)(goff[t] >= frame_bytes) + (int)(goff[t] >= 2u * frame_bytes) + (int)(goff[t] >= 3u * frame_bytes);
        const int delta = cam_delta[cam];
        // the 4 texels of the group as dwords (byte 3 is ignored), shifted, and packed back into the 12 bytes
        uint32_t P[4] = {w[0], __builtin_amdgcn_alignbyte(w[1], w[0], 3), __builtin_amdgcn_alignbyte(w[2], w[1], 2), w[2] >> 8};
        if (Src<SRC>::yuv) nv12_row_bgr<4>(w[0], w[1], P);
#pragma unroll
        for (int k = 0; k < 4; ++k) P[k] = luminance_shift_bgr(P[k], delta, hsv);
        uint32_t o[3];
        pack_pixels(P, o[0], o[1], o[2]);
        AlignedU3 ov; ov.x = o[0]; ov.y = o[1]; ov.z = o[2];
        *reinterpret_cast<AlignedU3 *>(fout + (size_t)gi * 12) = ov;
    }
