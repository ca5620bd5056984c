// The body of the backward's tile kernel, included AS TEXT (no include guard, not a function) by every kernel that runs
// it: mlp.hip's mlp_backward_kernel, mlp_chain.h's mlp_backward_tiles<T> (the bank) and mlp_joined.hip's
// mlp_joined_backward_kernel.  Called as a function at three tiles the register allocator no longer fits it into the 512
// VGPRs (mlp.hip: 488 and none spilled as text, 512 and 32 spilled as a call), hence text; one text, so that a change to
// the chain is a change to every kernel.
//
// In scope where it is included: int64_t N, tiles; const MlpNet& n (staged: mlp_stage has run); const MlpGrads& out (its
// g_W / g_b; out.g_x is the includer's business).  The includer defines, and undefines afterwards:
//   MLP_BODY_T                          accumulator tiles per layer side (a constant expression)
//   MLP_BODY_LDS                        the workgroup's LDS (float*): the images, then the waves' regions at n.wave_off
//   MLP_BODY_LOAD_X(a, row, live, g)    a_0 of this lane's row into f4 a[MLP_TILES], in mlp_load_rows's layout
//   MLP_BODY_LOAD_GY(d, row, live, g)   dZ of the last layer, likewise
//   MLP_BODY_WANT_DA0                   whether dA_0 is wanted (wave-uniform)
//   MLP_BODY_STORE_DA0(d, row, live, g) what becomes of dA_0 (f4 d[MLP_TILES]); `acts` (tile 0 = a_0) and `own` are in scope
//   MLP_BODY_RECORDS                    where the records start (float*): this wave's is at [first * n.P]
// A wave without a tile (only past the last tile's wave) returns from the kernel without a record.
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    float* __restrict__ acts = MLP_BODY_LDS + n.wave_off + wave * (n.L + 1) * 16 * MLP_ROW;      // a_l: tile l; dZ: tile L
    float* __restrict__ dz_t = acts + n.L * 16 * MLP_ROW;
    const int own = r * MLP_ROW + 4 * g;       // where this lane's four features of feature tile 0 lie in a tile

    f4 acc_w[PIGS_MLP_MAX_LAYERS][MLP_BODY_T][MLP_BODY_T], acc_b[PIGS_MLP_MAX_LAYERS][MLP_BODY_T];
#pragma unroll
    for (int l = 0; l < PIGS_MLP_MAX_LAYERS; ++l)
#pragma unroll
        for (int to = 0; to < MLP_BODY_T; ++to) {
            acc_b[l][to] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ti = 0; ti < MLP_BODY_T; ++ti) acc_w[l][to][ti] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        }

    const int64_t first = (int64_t)blockIdx.x * MLP_WAVES + wave, stride = (int64_t)gridDim.x * MLP_WAVES;
    for (int64_t tile = first; tile < tiles; tile += stride) {
        const int64_t row = tile * 16 + r;
        const bool live = row < N;
        f4 a[MLP_TILES], d[MLP_TILES];
        mlp_wave_fence();                      // the previous tile's reads of this region are done
        MLP_BODY_LOAD_X(a, row, live, g);
        for (int l = 0; l < n.L; ++l) {        // a_l to LDS, then a_{l+1}; y itself is not needed
#pragma unroll
            for (int t = 0; t < MLP_TILES; ++t) *reinterpret_cast<f4*>(acts + l * 16 * MLP_ROW + own + 16 * t) = a[t];
            if (l + 1 < n.L) {
                const int nti = mlp_tiles(n.w[l]), nto = mlp_tiles(n.w[l + 1]);
                mlp_layer(d, a, MLP_BODY_LDS + n.woff[l], MLP_BODY_LDS + n.boff[l], 16 * nti + 4, nti, nto, r, g);
                mlp_tanh(a, d);
            }
        }
        MLP_BODY_LOAD_GY(d, row, live, g);     // dZ of the last layer
#pragma unroll
        for (int l = PIGS_MLP_MAX_LAYERS - 1; l >= 0; --l) {
            if (l >= n.L) continue;
            const bool want_da = l > 0 || (MLP_BODY_WANT_DA0);
            mlp_backward_layer<MLP_BODY_T, MLP_BODY_T>(d, acc_w[l], acc_b[l], out.g_W[l] != nullptr, out.g_b[l] != nullptr,
                                                       want_da, l == 0, MLP_BODY_LDS + n.woff[l], mlp_tiles(n.w[l + 1]),
                                                       mlp_tiles(n.w[l]), acts + l * 16 * MLP_ROW, dz_t, own, r, g);
            if (l == 0 && want_da) { MLP_BODY_STORE_DA0(d, row, live, g); }
        }
    }

    // this wave's record; a wave without a tile (only past the last tile's wave) writes none
    if (first >= tiles) return;
    float* __restrict__ rec = (MLP_BODY_RECORDS) + first * n.P;
#pragma unroll
    for (int l = 0; l < PIGS_MLP_MAX_LAYERS; ++l) {
        if (l >= n.L) continue;
        mlp_record_layer<MLP_BODY_T, MLP_BODY_T>(rec, n.poff[l], acc_w[l], acc_b[l], out.g_W[l] != nullptr,
                                                 out.g_b[l] != nullptr, n.w[l], n.w[l + 1], r, g);
    }
