// libhotmi355x — the body of k_g2p (transfer.hip), included by its two overloads: the kernel of hot_config.plasticity (PLASTIC 0 / 1 / 2: one mapping for
// every particle) and the kernel of the per-particle classes (PLASTIC 3: pcls = the particles' classes, cls_tab = the context's 16 x 8 parameter table).
// Text, not a device function both call: wrapped in one, k_g2p<double, 0, true> — the instantiation every elastic step runs — came out of the register
// allocator with 26 spilled registers where this text in the kernel itself has none (160 VGPRs, profiles/kernel_resources.txt).
// Names the including kernel provides: its arguments, and pcls / cls_tab (null where PLASTIC < 3), yield_stress / sn0 .. sn4 (0 where PLASTIC == 3).
    using G = Geo<T>;
    constexpr int TY = G::BY + 2, TZ = G::BZ + 2, TILE = (G::BX + 2) * TY * TZ;
    __shared__ T nv[3][TILE];
    __shared__ T ptab[PLASTIC == 3 ? PCLS_MAX * PCLS_STRIDE : 1]; // the class parameters, copied beside the tile gather (PLASTIC == 3 only; otherwise never touched)
    const int g = blockIdx.x;
    const int first = group_first[g], last = group_first[g + 1];
    // the position of this thread's first particle is requested before the tile gather, and the tile's DOF ids come from the per-group
    // table (tileDof) instead of the nb8 -> gIdx chain: the workgroup's dependent round trips (indices -> nodal values, particle data)
    // run side by side.  Fn is NOT held across the 27-node loop (round 3: with it the fp64 kernel needed 214 registers, two wavefronts
    // per SIMD; it is read after the loop, when only the 21 sums are live, and the other wavefronts cover that round trip).
    const int p0 = first + threadIdx.x;
    T xpre[3] = { 0, 0, 0 };
    if (p0 < last) {
#pragma unroll
        for (int d = 0; d < 3; ++d) xpre[d] = X[(int64_t)d * Np + p0];
    }
    for (int t = threadIdx.x; t < TILE; t += 256) {
        int idx = gIdx[(int64_t)g * TILE + t]; // gIdx here = tileDof
        T a = 0, b = 0, c = 0;
        if (idx >= 0) {
            a = nodeV[3 * idx] + dv[3 * idx], b = nodeV[3 * idx + 1] + dv[3 * idx + 1], c = nodeV[3 * idx + 2] + dv[3 * idx + 2];
        }
        nv[0][t] = a, nv[1][t] = b, nv[2][t] = c;
    }
    if constexpr (PLASTIC == 3) {
        if (threadIdx.x < PCLS_MAX * PCLS_STRIDE) ptab[threadIdx.x] = cls_tab[threadIdx.x];
    }
    __syncthreads();
    const int ox = group_origin[3 * g], oy = group_origin[3 * g + 1], oz = group_origin[3 * g + 2];
    const T D_inverse = (T)4 / (dx * dx);
    int myflags = 0;
    for (int p = first + threadIdx.x; p < last; p += 256) {
        T xp[3];
        if (p == p0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) xp[d] = xpre[d];
        }
        else { // groups of more than 256 particles
#pragma unroll
            for (int d = 0; d < 3; ++d) xp[d] = X[(int64_t)d * Np + p];
        }
        int base[3];
        T w[3][3], dw[3][3];
#pragma unroll
        for (int d = 0; d < 3; ++d) bspline<T>(one_over_dx, xp[d], base[d], w[d], dw[d]);
        const int cx = base[0] - ox, cy = base[1] - oy, cz = base[2] - oz;
        T pic[3] = { 0, 0, 0 };
        T B[9], gv[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) B[c] = (T)0, gv[c] = (T)0;
        if constexpr (FACT) {
            T wz[3], wd2[3], dwz[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) wz[k] = w[2][k], wd2[k] = w[2][k] * ((T)(base[2] + k) * dx - xp[2]), dwz[k] = one_over_dx * dw[2][k];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const T wi = w[0][i], dwi = one_over_dx * dw[0][i];
                const T d0 = (T)(base[0] + i) * dx - xp[0];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int t = ((cx + i) * TY + (cy + j)) * TZ + cz;
                    T s0[3], s1[3], s2[3]; // column sums: sum_k w_k v, sum_k w_k d2_k v, sum_k dw_k / dx v
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const T va = nv[c][t], vb = nv[c][t + 1], vc = nv[c][t + 2];
                        s0[c] = fma(wz[2], vc, fma(wz[1], vb, wz[0] * va));
                        s1[c] = fma(wd2[2], vc, fma(wd2[1], vb, wd2[0] * va));
                        s2[c] = fma(dwz[2], vc, fma(dwz[1], vb, dwz[0] * va));
                    }
                    const T wij = wi * w[1][j], gi = dwi * w[1][j], gj = wi * (one_over_dx * dw[1][j]);
                    const T d1 = (T)(base[1] + j) * dx - xp[1];
                    const T a0 = wij * d0, a1 = wij * d1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        pic[c] = fma(wij, s0[c], pic[c]);
                        B[c] = fma(a0, s0[c], B[c]), B[3 + c] = fma(a1, s0[c], B[3 + c]), B[6 + c] = fma(wij, s1[c], B[6 + c]);
                        gv[c] = fma(gi, s0[c], gv[c]), gv[3 + c] = fma(gj, s0[c], gv[3 + c]), gv[6 + c] = fma(wij, s2[c], gv[6 + c]);
                    }
                }
            }
        }
        else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            T wi = w[0][i], dwi = one_over_dx * dw[0][i];
            T d0 = (T)(base[0] + i) * dx - xp[0];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                T wij = wi * w[1][j];
                T dwij_i = dwi * w[1][j], dwij_j = wi * one_over_dx * dw[1][j];
                T d1 = (T)(base[1] + j) * dx - xp[1];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    T wijk = wij * w[2][k];
                    T g0 = dwij_i * w[2][k], g1 = dwij_j * w[2][k], g2 = wij * one_over_dx * dw[2][k];
                    T d2 = (T)(base[2] + k) * dx - xp[2];
                    int t = ((cx + i) * TY + (cy + j)) * TZ + (cz + k);
                    T v0 = nv[0][t], v1 = nv[1][t], v2 = nv[2][t];
                    pic[0] += wijk * v0, pic[1] += wijk * v1, pic[2] += wijk * v2;
                    T wv0 = wijk * v0, wv1 = wijk * v1, wv2 = wijk * v2;
                    B[0] += wv0 * d0, B[1] += wv1 * d0, B[2] += wv2 * d0;
                    B[3] += wv0 * d1, B[4] += wv1 * d1, B[5] += wv2 * d1;
                    B[6] += wv0 * d2, B[7] += wv1 * d2, B[8] += wv2 * d2;
                    gv[0] += v0 * g0, gv[1] += v1 * g0, gv[2] += v2 * g0;
                    gv[3] += v0 * g1, gv[4] += v1 * g1, gv[5] += v2 * g1;
                    gv[6] += v0 * g2, gv[7] += v1 * g2, gv[8] += v2 * g2;
                }
            }
        }
        }
        Mat3<T> Fo;
#pragma unroll
        for (int c = 0; c < 9; ++c) Fo.a[c] = Fn[(int64_t)c * Np + p];
        V[p] = pic[0], V[Np + p] = pic[1], V[2 * Np + p] = pic[2];
        T ra = (apic_r + (T)1) * (T)0.5, rb = (apic_r - (T)1) * (T)0.5;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) C[(int64_t)(c * 3 + r) * Np + p] = ra * (B[c * 3 + r] * D_inverse) + rb * (B[r * 3 + c] * D_inverse);
        T inc0 = dt * pic[0], inc1 = dt * pic[1], inc2 = dt * pic[2];
        X[p] = xp[0] + inc0, X[Np + p] = xp[1] + inc1, X[2 * Np + p] = xp[2] + inc2;
        T inc = inc0 * inc0 + inc1 * inc1 + inc2 * inc2, dx2 = dx * dx;
        if (inc > dx2) myflags |= 1;
        if (inc > dx2 * (T)0.25 * (cfl * cfl)) myflags |= 2;
        if (gradV_out)
#pragma unroll
            for (int c = 0; c < 9; ++c) gradV_out[(int64_t)c * Np + p] = gv[c];
        // F = (I + dt gradV) Fn   (restoreStrain + evolveStrain)
        Mat3<T> A, Fnew;
#pragma unroll
        for (int c = 0; c < 9; ++c) A.a[c] = dt * gv[c] + ((c % 4 == 0) ? (T)1 : (T)0);
        Fnew = m3_mul(A, Fo);
        if (PLASTIC == 1) {
            von_mises_project(Fnew, Mu[p], Lam[p], yield_stress);
        }
        else if (PLASTIC == 2) {
            T mu = Mu[p], la = Lam[p], jp = Jp[p];
            snow_project(Fnew, mu, la, jp, sn0, sn1, sn2, sn3, sn4);
            Mu[p] = mu, Lam[p] = la, Jp[p] = jp;
        }
        else if constexpr (PLASTIC == 3) { // the class is loaded here, after the 27-node loop, when only Fnew is live (see Fn above)
            T mu = 0, la = 0, jp = 0;
            bool hardened;
            plasticity_classes_project(Fnew, &ptab[PCLS_STRIDE * pcls[p]], Mu, Lam, Jp, (int64_t)p, mu, la, jp, hardened);
            if (hardened) Mu[p] = mu, Lam[p] = la, Jp[p] = jp; // lanes of kind 2 only
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) F[(int64_t)c * Np + p] = Fnew.a[c];
    }
    // one global atomic per wavefront at most (2 M same-address atomics cost more than the whole transfer)
    unsigned long long m1 = __ballot(myflags & 1), m2 = __ballot(myflags & 2);
    if ((threadIdx.x & 63) == 0 && (m1 | m2)) {
        int bits = (m1 ? 1 : 0) | (m2 ? 2 : 0);
        int cur = __hip_atomic_load(flags_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((cur & bits) != bits) atomicOr(flags_out, bits); // already-set bits need no further traffic
    }
