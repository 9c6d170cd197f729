// pdlp_ruiz.inc -- the entry points that take no handle: the building blocks of Ruiz scaling over a CSR matrix (row factors, row
// and column division), the pdlp_vec_* vector helpers of the preconditioner and the report, and the two bandwidth probes
// (pdlp_probe_stream_read, pdlp_probe_gather).  Each is its argument checks and its launches, in the element type `dtype` names.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: grid_for, align_up, WITH_T, HIP_TRY
// (pdlp_hip.hip) and the kernels of pdlp_kernels_small.inc.
// ------------------------------------------------------------------------------------------------
extern "C" {

int pdlp_csr_row_scale_factors(int dtype, int64_t rows, const int64_t* rowptr, const void* val, double eps, void* norm, void* stream)
{
    if (rows < 0 || (dtype != PDLP_F32 && dtype != PDLP_F64)) return PDLP_ERR_INVALID;
    if (rows == 0) return PDLP_OK;
    const int g = grid_for(rows * 8);
    WITH_T(dtype, hipLaunchKernelGGL(k_row_scale_factors<T>, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, rows, rowptr, (const T*)val, (T)eps,
                                     (T*)norm));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_csr_row_l1_factors(int dtype, int64_t rows, const int64_t* rowptr, const void* val, void* norm, void* stream)
{
    if (rows < 0 || (dtype != PDLP_F32 && dtype != PDLP_F64) || (rows > 0 && (!rowptr || !norm))) return PDLP_ERR_INVALID;
    if (rows == 0) return PDLP_OK;
    const int g = grid_for(rows * 8);
    WITH_T(dtype, hipLaunchKernelGGL(k_row_l1_factors<T>, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, rows, rowptr, (const T*)val, (T*)norm));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_csr_div_rows(int dtype, int64_t rows, const int64_t* rowptr, void* val, const void* norm, void* stream)
{
    if (rows < 0 || (dtype != PDLP_F32 && dtype != PDLP_F64)) return PDLP_ERR_INVALID;
    if (rows == 0) return PDLP_OK;
    const int g = grid_for(rows * 8);
    WITH_T(dtype, hipLaunchKernelGGL(k_div_rows<T>, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, rows, rowptr, (T*)val, (const T*)norm));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_csr_div_cols(int dtype, int64_t nnz, const int32_t* colidx, void* val, const void* norm_full, void* stream)
{
    if (nnz < 0 || (dtype != PDLP_F32 && dtype != PDLP_F64)) return PDLP_ERR_INVALID;
    if (nnz == 0) return PDLP_OK;
    const int g = grid_for(nnz);
    WITH_T(dtype, hipLaunchKernelGGL(k_div_cols<T>, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, nnz, colidx, (T*)val, (const T*)norm_full));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_vec_muldiv(int dtype, int64_t len, void* a, const void* b, int op, void* stream)
{
    if (len < 0 || (dtype != PDLP_F32 && dtype != PDLP_F64) || (op != 0 && op != 1)) return PDLP_ERR_INVALID;
    if (len == 0) return PDLP_OK;
    WITH_T(dtype, hipLaunchKernelGGL(k_muldiv<T>, dim3(grid_for(len)), dim3(BLOCK), 0, (hipStream_t)stream, len, (T*)a, (const T*)b, op));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_vec_project_lambda(int dtype, int64_t len, const void* g, const void* l, const void* u, void* out, void* stream)
{
    if ((dtype != PDLP_F32 && dtype != PDLP_F64) || len < 0 || (len > 0 && (!g || !l || !u || !out))) return PDLP_ERR_INVALID;
    if (len == 0) return PDLP_OK;
    WITH_T(dtype, hipLaunchKernelGGL(k_project_lambda<T>, dim3(grid_for(len)), dim3(BLOCK), 0, (hipStream_t)stream, len, (const T*)g, (const T*)l,
                                     (const T*)u, (T*)out));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_vec_max_dev_from_one(int dtype, int64_t len, const void* v, void* work8, double* out, void* stream)
{
    if (len < 0 || !work8 || !out || (dtype != PDLP_F32 && dtype != PDLP_F64)) return PDLP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(work8, 0, 8, s));
    if (len > 0) {
        WITH_T(dtype, hipLaunchKernelGGL(k_max_dev_from_one<T>, dim3(grid_for(len)), dim3(BLOCK), 0, s, len, (const T*)v, (double*)work8));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(out, work8, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return PDLP_OK;
}

int pdlp_vec_sqdist(int dtype, int64_t len, const void* a, const void* b, void* work, double* out, void* stream)
{
    if (len < 0 || !work || !out || (len > 0 && (!a || !b)) || (dtype != PDLP_F32 && dtype != PDLP_F64)) return PDLP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    *out = 0.0;
    if (len == 0) return PDLP_OK;
    // partial sums of <= 256 workgroups at work[b * NACC], added in fixed order by one workgroup into work[256 * NACC]
    const int64_t want = (len + BLOCK - 1) / BLOCK;
    const int grid = (int)(want < 256 ? want : 256);
    double* part = (double*)work;
    WITH_T(dtype, hipLaunchKernelGGL(k_sqdiff<T>, dim3(grid), dim3(BLOCK), 0, s, len, (const T*)a, (const T*)b, part));
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, s, (const double*)part, grid, 1, part + 256 * NACC, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, part + 256 * NACC, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return PDLP_OK;
}

int pdlp_probe_stream_read(const void* buf, int64_t bytes, int reps, void* stream, double* gb_per_s)
{
    if (!buf || bytes < ((int64_t)1 << 24) || reps < 1 || !gb_per_s || ((uintptr_t)buf & 15u)) return PDLP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t n16 = (size_t)bytes / 16;
    const int grid = 512;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    unsigned* sink = (unsigned*)const_cast<void*>(buf);           // (never written: see the kernel)
    hipLaunchKernelGGL(k_probe_read, dim3(grid), dim3(512), 0, s, (const probe_u32x4*)buf, n16, sink);
    HIP_TRY(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_probe_read, dim3(grid), dim3(512), 0, s, (const probe_u32x4*)buf, n16, sink);
    HIP_TRY(hipEventRecord(e1, s));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIP_TRY(hipGetLastError());
    const size_t per = n16 / grid, read16 = per / (4 * 512) * (4 * 512) * grid;      // what the kernel really loads
    *gb_per_s = (double)read16 * 16.0 * reps / ((double)ms * 1e-3) / 1e9;
    return PDLP_OK;
}

int pdlp_probe_gather(void* scratch, int64_t scratch_bytes, int64_t table_entries, int reps, void* stream, double* gitems_per_s)
{
    if (!scratch || table_entries < 1 || table_entries > (int64_t)1 << 31 || reps < 1 || !gitems_per_s || ((uintptr_t)scratch & 255u))
        return PDLP_ERR_INVALID;
    const int64_t tbytes = align_up(table_entries * 4 + 256, 256);
    const int64_t items = (scratch_bytes - tbytes) / 8 / NNZ_CAP * NNZ_CAP;
    if (items < (int64_t)NNZ_CAP * 64) return PDLP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    float* table = (float*)scratch;
    uint32_t* idx = (uint32_t*)((char*)scratch + tbytes);
    float* val = (float*)(idx + items);
    HIP_TRY(hipMemsetAsync(table, 0, (size_t)tbytes, s));
    hipLaunchKernelGGL(k_probe_fill, dim3(grid_for(items)), dim3(BLOCK), 0, s, idx, val, items, (uint32_t)table_entries);
    const int64_t nblk = items / NNZ_CAP;
    const int grid = (int)(nblk < MAX_GRID ? nblk : MAX_GRID);
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    float* sink = table + table_entries;               // (inside the padding of the table; never written)
    hipLaunchKernelGGL(k_probe_gather, dim3(grid), dim3(BLOCK), 0, s, idx, val, table, items, sink);
    HIP_TRY(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_probe_gather, dim3(grid), dim3(BLOCK), 0, s, idx, val, table, items, sink);
    HIP_TRY(hipEventRecord(e1, s));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIP_TRY(hipGetLastError());
    *gitems_per_s = (double)items * reps / ((double)ms * 1e-3) / 1e9;
    return PDLP_OK;
}

}  // extern "C"
