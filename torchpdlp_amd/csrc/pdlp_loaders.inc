// pdlp_loaders.inc -- the two libraries resolved at run time with dlopen, so that the library links against neither: RCCL (g_rccl,
// rccl_load, RCCL_TRY; single-GPU use never touches it) and roctx (g_roctx, roctx_load, the scoped Range), with the
// pdlp_trace_enable / pdlp_range_push / pdlp_range_pop entry points.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: HIP_TRY and the headers (pdlp_hip.hip).
// ------------------------------------------------------------------------------------------------
namespace {

// ------------------------------------------------------------------------------------------------
// RCCL, resolved at run time (single-GPU use never touches it)
// ------------------------------------------------------------------------------------------------
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;            // optional (chunked exchange): grouped in-place broadcasts
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    int last_error = 0;
};
Rccl g_rccl;

int rccl_load(const char* path)
{
    if (g_rccl.lib) return PDLP_OK;
    const char* names[] = {path, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* lib = nullptr;
    for (const char* nm : names) {
        if (!nm || !*nm) continue;
        lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
    }
    if (!lib) return PDLP_ERR_COMM;
    Rccl r;
    r.lib = lib;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(lib, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(lib, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(lib, "ncclAllGather");
    r.AllReduce = (decltype(r.AllReduce))dlsym(lib, "ncclAllReduce");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(lib, "ncclGetErrorString");
    r.Broadcast = (decltype(r.Broadcast))dlsym(lib, "ncclBroadcast");
    r.GroupStart = (decltype(r.GroupStart))dlsym(lib, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(lib, "ncclGroupEnd");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.AllReduce) return PDLP_ERR_COMM;
    g_rccl = r;
    return PDLP_OK;
}

#define RCCL_TRY(expr)                                       \
    do {                                                     \
        ncclResult_t r_ = (expr);                            \
        if (r_ != ncclSuccess) { g_rccl.last_error = (int)r_; return PDLP_ERR_COMM; } \
    } while (0)

// ------------------------------------------------------------------------------------------------
// roctx ranges (rocprofv3 --marker-trace): the counterpart of the reference's Timer (PDLP/util.py:6-27, wall-clock sections printed at
// the end of a run).  Resolved with dlopen on first use after pdlp_trace_enable -- no link-time dependency, nothing happens when
// tracing is off.  Level 2 also synchronises the given stream at both ends of a range, so that the range's wall time IS the
// GPU time of what was enqueued inside it (the per-phase table of profiles/README.md); level 1 marks the host side only.
// ------------------------------------------------------------------------------------------------
struct Roctx {
    int level = 0;
    bool tried = false;
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
Roctx g_roctx;

void roctx_load()
{
    if (g_roctx.tried) return;
    g_roctx.tried = true;
    const char* names[] = {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/librocprofiler-sdk-roctx.so",
                           "libroctx64.so", "libroctx64.so.4", "/opt/rocm/lib/libroctx64.so"};
    for (const char* nm : names) {
        void* lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) continue;
        g_roctx.push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
        g_roctx.pop = (int (*)())dlsym(lib, "roctxRangePop");
        if (g_roctx.push && g_roctx.pop) return;
        g_roctx.push = nullptr; g_roctx.pop = nullptr;
    }
}

struct Range {         // scoped range on the handle's stream
    hipStream_t s;
    bool on;
    Range(const char* name, hipStream_t stream) : s(stream), on(g_roctx.level > 0 && g_roctx.push)
    {
        if (!on) return;
        if (g_roctx.level > 1) (void)hipStreamSynchronize(s);
        (void)g_roctx.push(name);
    }
    ~Range()
    {
        if (!on) return;
        if (g_roctx.level > 1) (void)hipStreamSynchronize(s);
        (void)g_roctx.pop();
    }
};

}  // namespace

extern "C" {

int pdlp_trace_enable(int level)
{
    if (level < 0 || level > 2) return PDLP_ERR_INVALID;
    if (level > 0) {
        roctx_load();
        if (!g_roctx.push) { g_roctx.level = 0; return PDLP_ERR_STATE; }       // no roctx library on this machine
    }
    g_roctx.level = level;
    return PDLP_OK;
}

int pdlp_range_push(const char* name, void* stream)
{
    if (!name) return PDLP_ERR_INVALID;
    if (g_roctx.level > 0 && g_roctx.push) {
        if (g_roctx.level > 1) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        (void)g_roctx.push(name);
    }
    return PDLP_OK;
}

int pdlp_range_pop(void* stream)
{
    if (g_roctx.level > 0 && g_roctx.pop) {
        if (g_roctx.level > 1) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        (void)g_roctx.pop();
    }
    return PDLP_OK;
}

}  // extern "C"
