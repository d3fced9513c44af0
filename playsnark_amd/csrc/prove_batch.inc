// ps_groth16_prove_batch: k proofs under one Lagrange-form key in one call (included by capi.hip behind prove.inc;
// kernels in prove_batch.hpp, the sums in msm_batch.inc).
//
// The Lagrange-form route has no interpolation and no division: the sums' scalars are the wire values themselves and the
// values of h on the nodes n+1..2n-1, so a witness that violates a gate yields garbage scalars and no fault, and nothing on
// the host has to look at a witness before the next one is enqueued.  Per call, all on the context stream:
//   1  k_fr_to_mont over the k * m witness values, k_spmv_batch (+ k_spmv_long_rows_batch) -> y[3][k][n], k_check_gates_batch
//      -> k flags
//   2  the rows of SA [k][n+2], SB [k][n+2], SC [k][nn + (n-1) + n + 3] (the unsplit layout of g16_quotient_stage) but for h
//   3  per witness quotient_h_values on the circuit's scratch, back to back, each into row j of SC
//   4  ONE read of the flags, then three ps_msm_batch sums over the prover's cached arrays PB, PA, PC
// The proof bytes do not depend on the single prover's split forms (PS_G16_B1_MIN_N, an int64 witness's NioLP part): those
// change how C is summed, not its value.

// stages of the last timed call (ps_ctx_set_timing): wires + gate check + rows, h values, then the three sums B, A, C
static int g16b_mark(ps_ctx* c, hipEvent_t* ev, int i) {
    if (!c->timing) return PS_OK;
    if (!ev[i]) HIP_TRY(hipEventCreate(&ev[i]));
    HIP_TRY(hipEventRecord(ev[i], c->stream));
    return PS_OK;
}

extern "C" int ps_groth16_prove_batch(ps_ctx* c, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sols, size_t k,
                                      const uint8_t* r_be32, const uint8_t* s_be32, uint8_t* A_out, uint8_t* B_out, uint8_t* C_out,
                                      int* valid) {
    if (!c || !pk || !q || !sols) return fail(PS_ERR_ARG, "ps_groth16_prove_batch: NULL argument");
    if (k && (!r_be32 || !s_be32 || !A_out || !B_out || !C_out)) return fail(PS_ERR_ARG, "ps_groth16_prove_batch: NULL argument");
    if (!pk->nio_lp) return fail(PS_ERR_ARG, "ps_groth16_prove_batch: NULL CRS array");
    if (!g16_lagrange(pk))
        return fail(PS_ERR_ARG, "ps_groth16_prove_batch: needs a Lagrange-form key (lxi, lxi2, lxi_t; ps_points_monomial_to_lagrange makes them)");
    const size_t n = q->n, m = q->m;
    const size_t diff = m - q->nio;               // groth16.go:175
    const size_t nn = ps_points_len(pk->nio_lp);  // groth16.go:176
    if (sols->n != k * m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");  // sanityCheck, qap.go:177-189
    if (diff + nn > m) return fail(PS_ERR_LENGTH, "NioLP longer than the non-IO part of the solution");
    if (n < 2) return fail(PS_ERR_ARG, "ps_groth16_prove_batch: needs at least 2 gates");
    if (ctx_busy(c)) return fail(PS_ERR_ARG, "ps_groth16_prove_batch: an MSM is pending on this context");
    if (k == 0) return PS_OK;
    const size_t LC = nn + (n - 1) + n + 3;
    if ((u64)k * LC >= (1ull << 31) || (u64)k * m >= (1ull << 31)) return fail(PS_ERR_ARG, "ps_groth16_prove_batch: batch too long (split it)");
    HIP_TRY(hipSetDevice(c->device));
    const auto t_start = std::chrono::steady_clock::now();
    int rc = groth16_prepare(c, pk, n, nn, false);
    if (rc) return rc;
    // r_j, s_j, r_j s_j as plain limbs, then room for the k gate flags
    std::vector<u32> small(24 * k);
    for (size_t j = 0; j < k; j++) {
        const Fr rm = fr_mont_from_be32(r_be32 + 32 * j), sm = fr_mont_from_be32(s_be32 + 32 * j);
        fr_to_words8(&small[24 * j], fr_from_mont(rm));
        fr_to_words8(&small[24 * j + 8], fr_from_mont(sm));
        fr_to_words8(&small[24 * j + 16], fr_from_mont(fr_mul(rm, sm)));
    }
    ps_scalars *SA = nullptr, *SB = nullptr, *SC = nullptr;  // the context's own (prover_vector): not freed here
    if ((rc = prover_vector(c, 0, k * (n + 2), &SA)) || (rc = prover_vector(c, 1, k * (n + 2), &SB)) || (rc = prover_vector(c, 2, k * LC, &SC)))
        return rc;
    if ((rc = c->pb_x.ensure(sizeof(Fr) * k * m)) || (rc = c->pb_y.ensure(sizeof(Fr) * 3 * k * n)) || (rc = c->pb_small.ensure(4 * (24 * k + k))))
        return rc;
    Fr* X = (Fr*)c->pb_x.p;
    Fr* Y = (Fr*)c->pb_y.p;
    u32* d_small = (u32*)c->pb_small.p;
    u32* d_flags = d_small + 24 * k;
    hipStream_t st = c->stream;
    const NttTables& tabs = *ctx_tabs(c);
    if (storage_wait_ready(sols->st, st)) return fail(PS_ERR_HIP, "ps_groth16_prove_batch: event wait failed");
    if ((rc = g16b_mark(c, c->pb_ev, 0))) return rc;
    HIP_TRY(hipMemcpyAsync(d_small, small.data(), 4 * small.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_flags, 0, 4 * k, st));
    // 1: wire values and the gate check of every witness
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk((u64)k * m)), dim3(256), 0, st, X, scalars_ptr(sols), (u64)k * m);
    Csr3 m3;
    for (int i = 0; i < 3; i++) m3.m[i] = CsrView{q->mat[i].row_ptr, q->mat[i].col, q->mat[i].val};
    hipLaunchKernelGGL(k_spmv_batch, dim3(nblk((u64)k * n), 3), dim3(256), 0, st, m3, (const Fr*)X, (u32)m, (u32)n, (u32)k, Y);
    for (int i = 0; i < 3; i++)
        if (q->mat[i].n_long)
            hipLaunchKernelGGL(k_spmv_long_rows_batch, dim3((unsigned)((u64)q->mat[i].n_long * k)), dim3(256), 0, st, q->mat[i].row_ptr, q->mat[i].col,
                               q->mat[i].val, (const Fr*)X, (u32)m, (u32)n, Y + (size_t)i * k * n, q->mat[i].long_rows, q->mat[i].n_long);
    hipLaunchKernelGGL(k_check_gates_batch, dim3(nblk((u64)k * n)), dim3(256), 0, st, (const Fr*)Y, (u32)n, (u32)k, d_flags);
    // 2: the scalar matrices but for h
    const Fr *yA = Y, *yB = Y + k * n, *yC = Y + 2 * k * n;
    u32 *sa = (u32*)SA->st->p, *sb = (u32*)SB->st->p, *sc = (u32*)SC->st->p;
    hipLaunchKernelGGL(k_g16b_fill_ab, dim3(nblk((u64)k * (n + 2))), dim3(256), 0, st, sa, yA, (const u32*)d_small, 0, (u32)n, (u32)k);
    hipLaunchKernelGGL(k_g16b_fill_ab, dim3(nblk((u64)k * (n + 2))), dim3(256), 0, st, sb, yB, (const u32*)d_small, 1, (u32)n, (u32)k);
    hipLaunchKernelGGL(k_g16b_fill_c, dim3(nblk((u64)k * (nn + n + 3))), dim3(256), 0, st, sc, scalars_ptr(sols), yA, yB, (const u32*)d_small,
                       (u32)n, (u32)nn, (u32)m, (u32)diff, (u32)k);
    HIP_TRY(hipGetLastError());
    if ((rc = g16b_mark(c, c->pb_ev, 1))) return rc;
    // 3: h on the nodes n+1..2n-1, witness by witness on the circuit's scratch (a batch of 3 k transforms is a follow-up)
    for (size_t j = 0; j < k; j++) {
        hipError_t e = quotient_h_values(tabs, st, q->qt, yA + j * n, yB + j * n, yC + j * n);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return fail(PS_ERR_HIP, std::string("ps_groth16_prove_batch: h values: ") + hipGetErrorString(e));
        }
        hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(n - 1)), dim3(256), 0, st, sc + 8 * (j * LC + nn), (const Fr*)q->qt.scratch, (u64)(n - 1));
    }
    HIP_TRY(hipGetLastError());
    if ((rc = g16b_mark(c, c->pb_ev, 2))) return rc;
    // 4: the flags, read once
    std::vector<u32> flags(k);
    if (hipMemcpyAsync(flags.data(), d_flags, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(PS_ERR_HIP, "ps_groth16_prove_batch: reading the gate checks failed");
    c->phase_ms[0] = ms_since(t_start);
    if (!valid)
        for (size_t j = 0; j < k; j++)
            if (flags[j]) return fail(PS_ERR_NOT_DIVISIBLE, "apocalypse: witness " + std::to_string(j) + " of the batch violates a gate");  // qap.go:158-160
    // B first, as the single prover launches them
    if ((rc = ps_msm_batch(c, c->g16_pb, SB, k, B_out))) return rc;
    if ((rc = g16b_mark(c, c->pb_ev, 3))) return rc;
    if ((rc = ps_msm_batch(c, c->g16_pa, SA, k, A_out))) return rc;
    if ((rc = g16b_mark(c, c->pb_ev, 4))) return rc;
    if ((rc = ps_msm_batch(c, c->g16_pc, SC, k, C_out))) return rc;
    if ((rc = g16b_mark(c, c->pb_ev, 5))) return rc;
    if (valid)
        for (size_t j = 0; j < k; j++) {
            valid[j] = flags[j] == 0;
            if (flags[j]) {
                memset(A_out + 96 * j, 0, 96);
                memset(B_out + 192 * j, 0, 192);
                memset(C_out + 96 * j, 0, 96);
            }
        }
    c->pb_timed = c->timing;
    c->phase_ms[1] = 0.f;
    c->phase_ms[3] = ms_since(t_start);
    c->phase_ms[2] = c->phase_ms[3] - c->phase_ms[0];
    return PS_OK;
}
