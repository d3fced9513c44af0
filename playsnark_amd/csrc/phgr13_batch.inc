// ps_phgr13_prove_batch: k proofs under one evaluation key in one call (included by capi.hip behind prove_batch.inc; the
// kernels are those of ps_groth16_prove_batch, prove_batch.hpp; the sums are in msm_batch.inc).
//
// Seven of PHGR13's eight proof elements are sums over the same scalars, solution[diff:] (pinochio.go:231-241, with the three
// beta arrays summed pointwise once per key: phgr13_beta_sum), the eighth is h over the Lagrange form of gsi.  Per call:
//   1  k_fr_to_mont over the k * m witness values, k_spmv_batch (+ k_spmv_long_rows_batch) -> y[3][k][n], k_check_gates_batch
//      -> k flags; per witness quotient_h_values on the circuit's scratch, back to back, each into row j of H[k][n-1]
//   2  ONE read of the flags, then hs = ps_msm_batch(lgsi, H, k)
//   3  ONE ps_msm_batch_multi over {vs, ws, ys, vas, was, yas, beta sum} with scalars = the witnesses as they were uploaded
//      (stride m, first diff: plain limbs already, nothing is copied, the IO part of a witness is never read)
// all on the context stream but for the point passes and folds of step 3, which rotate over the context's workspaces.  The
// solution sums do not depend on h; they are nevertheless started behind the h sum: the h values occupy the chip with NTT
// passes, and a sort that shares the chip waits for CUs (prove_shares.inc, phgr13_share_sums).  The window tables are
// those of the single prover (prove_shares.inc: lgsi, the six solution arrays and the beta sum; a table that finds no room is
// no error), and both sums run over them where ps_msm_batch_set_table admits it (msm_batch.inc).

extern "C" int ps_phgr13_prove_batch(ps_ctx* c, const ps_phgr13_ek* ek, const ps_qap* q, const ps_scalars* sols, size_t k, ps_phgr13_proof* out,
                                     int* valid) {
    if (!c || !ek || !q || !sols || (k && !out)) return fail(PS_ERR_ARG, "ps_phgr13_prove_batch: NULL argument");
    int rc = phgr13_check_arrays(ek, "ps_phgr13_prove_batch");
    if (rc) return rc;
    if (!ek->lgsi)
        return fail(PS_ERR_ARG, "ps_phgr13_prove_batch: needs the Lagrange form of gsi in the key (lgsi; ps_points_monomial_to_lagrange makes it)");
    const size_t n = q->n, m = q->m;
    const size_t diff = m - q->nio;  // pinochio.go:219
    const size_t nn = ek->vs->n;
    for (const ps_points* p : {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, ek->vbs, ek->wbs, ek->ybs})
        if (p->n != nn) return fail(PS_ERR_LENGTH, "ps_phgr13_prove_batch: the nine solution arrays of the key differ in length");
    if (diff + nn > m) return fail(PS_ERR_LENGTH, "evaluation-key array longer than the non-IO part of the solution");
    if (n < 1 || ek->gsi->n != n - 1 || ek->lgsi->n != n - 1)  // hx.BlindEval(zeroG1, ek.gsi) panics, algebra.go:350-352
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(n ? n - 1 : 0) + " and blinded eval points " +
                                       std::to_string(ek->gsi->n != n - 1 ? ek->gsi->n : ek->lgsi->n));
    if (m && k > (size_t)-1 / m) return fail(PS_ERR_ARG, "ps_phgr13_prove_batch: batch too long (split it)");
    if (sols->n != k * m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");  // sanityCheck, qap.go:177-189
    if (n < 2) return fail(PS_ERR_ARG, "ps_phgr13_prove_batch: needs at least 2 gates");
    if (ctx_busy(c)) return fail(PS_ERR_ARG, "ps_phgr13_prove_batch: an MSM is pending on this context");
    if (k == 0) return PS_OK;
    if ((u64)k * m >= (1ull << 31) || (u64)k * (n - 1) >= (1ull << 31)) return fail(PS_ERR_ARG, "ps_phgr13_prove_batch: batch too long (split it)");
    HIP_TRY(hipSetDevice(c->device));
    const auto t_start = std::chrono::steady_clock::now();
    if (nn && (rc = phgr13_beta_sum(c, ek))) return rc;
    // the tables ps_phgr13_prove asks for, each by the length of the sum that reads it: the h sum of a batch runs over the
    // whole of lgsi however few solution entries the circuit has (nn = 3 for a circuit of three IO variables)
    if (nn && tables_wanted(c, nn) && (rc = phgr13_solution_tables(c, ek))) return rc;
    if (tables_wanted(c, ek->lgsi->n) && (rc = phgr13_h_table(c, ek->lgsi))) return rc;
    ps_scalars* H = nullptr;  // the context's own (prover_vector): not freed here
    if ((rc = prover_vector(c, 3, k * (n - 1), &H))) return rc;
    if ((rc = c->pb_x.ensure(sizeof(Fr) * k * m)) || (rc = c->pb_y.ensure(sizeof(Fr) * 3 * k * n)) || (rc = c->pb_small.ensure(4 * k))) return rc;
    Fr* X = (Fr*)c->pb_x.p;
    Fr* Y = (Fr*)c->pb_y.p;
    u32* d_flags = (u32*)c->pb_small.p;
    hipStream_t st = c->stream;
    const NttTables& tabs = *ctx_tabs(c);
    if (storage_wait_ready(sols->st, st)) return fail(PS_ERR_HIP, "ps_phgr13_prove_batch: event wait failed");
    HIP_TRY(hipMemsetAsync(d_flags, 0, 4 * k, st));
    // 1: wire values and the gate check of every witness, then h on the nodes n+1..2n-1 witness by witness
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk((u64)k * m)), dim3(256), 0, st, X, scalars_ptr(sols), (u64)k * m);
    Csr3 m3;
    for (int i = 0; i < 3; i++) m3.m[i] = CsrView{q->mat[i].row_ptr, q->mat[i].col, q->mat[i].val};
    hipLaunchKernelGGL(k_spmv_batch, dim3(nblk((u64)k * n), 3), dim3(256), 0, st, m3, (const Fr*)X, (u32)m, (u32)n, (u32)k, Y);
    for (int i = 0; i < 3; i++)
        if (q->mat[i].n_long)
            hipLaunchKernelGGL(k_spmv_long_rows_batch, dim3((unsigned)((u64)q->mat[i].n_long * k)), dim3(256), 0, st, q->mat[i].row_ptr, q->mat[i].col,
                               q->mat[i].val, (const Fr*)X, (u32)m, (u32)n, Y + (size_t)i * k * n, q->mat[i].long_rows, q->mat[i].n_long);
    hipLaunchKernelGGL(k_check_gates_batch, dim3(nblk((u64)k * n)), dim3(256), 0, st, (const Fr*)Y, (u32)n, (u32)k, d_flags);
    HIP_TRY(hipGetLastError());
    const Fr *yA = Y, *yB = Y + k * n, *yC = Y + 2 * k * n;
    u32* h = (u32*)H->st->p;
    for (size_t j = 0; j < k; j++) {
        hipError_t e = quotient_h_values(tabs, st, q->qt, yA + j * n, yB + j * n, yC + j * n);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return fail(PS_ERR_HIP, std::string("ps_phgr13_prove_batch: h values: ") + hipGetErrorString(e));
        }
        hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(n - 1)), dim3(256), 0, st, h + 8 * j * (n - 1), (const Fr*)q->qt.scratch, (u64)(n - 1));
    }
    if (hipGetLastError() != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(PS_ERR_HIP, "ps_phgr13_prove_batch: a kernel of the h values could not be launched");
    }
    // the flags, read once
    std::vector<u32> flags(k);
    if (hipMemcpyAsync(flags.data(), d_flags, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(PS_ERR_HIP, "ps_phgr13_prove_batch: reading the gate checks failed");
    c->phase_ms[0] = ms_since(t_start);
    if (!valid)
        for (size_t j = 0; j < k; j++)
            if (flags[j]) return fail(PS_ERR_NOT_DIVISIBLE, "apocalypse: witness " + std::to_string(j) + " of the batch violates a gate");  // qap.go:158-160
    // 2: hs := hx.BlindEval(zeroG1, ek.gsi), pinochio.go:218, over the Lagrange form
    const auto t_h = std::chrono::steady_clock::now();
    std::vector<uint8_t> hs(96 * k), sums(k * (6 * 96 + 192));
    if ((rc = ps_msm_batch(c, ek->lgsi, H, k, hs.data()))) return rc;
    c->phase_ms[1] = ms_since(t_h);
    // 3: the seven solution sums, computeSolCommit on solution[diff:] (pinochio.go:222-241)
    const auto t_sums = std::chrono::steady_clock::now();
    const ps_points* arr[7] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, nn ? c->phgr_bsum : ek->vbs};
    uint8_t* dst[7];
    {
        uint8_t* p = sums.data();
        for (int i = 0; i < 7; i++) {
            dst[i] = p;
            p += k * wire_bytes(arr[i]->group);
        }
    }
    if ((rc = ps_msm_batch_multi(c, arr, 7, sols, k, m, diff, dst))) return rc;
    for (size_t j = 0; j < k; j++) {
        ps_phgr13_proof* o = &out[j];
        if (flags[j]) {  // only with `valid`
            memset(o, 0, sizeof *o);
            continue;
        }
        uint8_t* field[7] = {o->vss, o->wss, o->yss, o->vass, o->wass, o->yass, o->gz};
        for (int i = 0; i < 7; i++) {
            const size_t wb = wire_bytes(arr[i]->group);
            memcpy(field[i], dst[i] + j * wb, wb);
        }
        memcpy(o->hs, hs.data() + 96 * j, 96);
    }
    if (valid)
        for (size_t j = 0; j < k; j++) valid[j] = flags[j] == 0;
    c->phase_ms[2] = ms_since(t_sums);
    c->phase_ms[3] = ms_since(t_start);
    return PS_OK;
}
