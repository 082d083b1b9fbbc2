// Saved environment states (fjsp_snapshot_*, include/fjsp_amd.h): two copy kernels between a batch's env slab /
// dispatch-record table and a snapshot buffer.
//
// Snapshot buffer (SnapBuf, fjsp_device.h), one hipMalloc:
//   [n][e_stride]   env records, entry-major (entry q = the record of env idx[q] at save time)
//   [n] int2        per-entry header {instance = env % n_inst, source env}; {-1, -1}: never saved / bad index
//   [cap][n] uint4  dispatch records, slot-major like the batch's [cap][N] table (fjsp_env_record_schedule)
//
// Each launch has two parts over one grid: blocks [0, nb_env) copy env records, 16 bytes per thread (one
// global_load_dwordx4 / global_store_dwordx4).  e_stride is a multiple of 128 bytes, so the 64 lanes of a wave move
// eight whole 128-byte lines, and a line never straddles two records.  The remaining blocks copy dispatch records,
// one 16-byte record per thread, consecutive threads over consecutive envs of one slot (coalesced over the env
// index, as launch_schedule_unpack reads them).  Nothing synchronises with the host.
#include <hip/hip_runtime.h>

#include "fjsp_device.h"

namespace fjsp {

namespace {

constexpr int kSnapBlock = 256;

__global__ __launch_bounds__(kSnapBlock) void snapshot_save_kernel(DevBatch b, SchedRec rec, SnapBuf s, const int32_t *idx,
                                                                   uint32_t nb_env) {
    const uint32_t W = b.L.e_stride / 16u;                          // uint4 per env record
    if (blockIdx.x < nb_env) {
        const uint32_t g = blockIdx.x * kSnapBlock + threadIdx.x;
        if (g >= (uint32_t)s.n * W) return;
        const uint32_t q = g / W, w = g - q * W;
        const int env = idx ? idx[q] : (int)q;
        const bool ok = env >= 0 && env < b.N;
        if (w == 0) {
            s.hdr[q] = ok ? make_int2(env % b.n_inst, env) : make_int2(-1, -1);
            if (!ok) atomicAdd(s.err, 1ull);
        }
        if (!ok) return;
        const uint4 *src = reinterpret_cast<const uint4 *>(b.envs) + (size_t)env * W;
        reinterpret_cast<uint4 *>(s.env)[(size_t)q * W + w] = src[w];
        return;
    }
    const uint32_t g = (blockIdx.x - nb_env) * kSnapBlock + threadIdx.x;
    if (g >= (uint32_t)s.cap * (uint32_t)s.n) return;
    const uint32_t slot = g / (uint32_t)s.n, q = g - slot * (uint32_t)s.n;
    const int env = idx ? idx[q] : (int)q;
    if (env < 0 || env >= b.N) return;
    s.rec[g] = rec.rec[(size_t)slot * (uint32_t)b.N + (uint32_t)env];
}

// entry e may be loaded into env i: it was saved, and from an env of the same instance
__device__ inline bool entry_fits(const SnapBuf &s, int e, int i, int n_inst) {
    return e >= 0 && e < s.n && s.hdr[e].x == i % n_inst;
}

__global__ __launch_bounds__(kSnapBlock) void snapshot_load_kernel(DevBatch b, SchedRec rec, SnapBuf s, const int32_t *src,
                                                                   uint32_t nb_env) {
    const uint32_t W = b.L.e_stride / 16u;
    if (blockIdx.x < nb_env) {
        const uint32_t g = blockIdx.x * kSnapBlock + threadIdx.x;
        if (g >= (uint32_t)b.N * W) return;
        const uint32_t i = g / W, w = g - i * W;
        const int e = src ? src[i] : ((int)i < s.n ? (int)i : -1);
        if (e < 0) return;                                          // -1: keep env i as it is
        if (!entry_fits(s, e, (int)i, b.n_inst)) {                  // never write an env of another instance
            if (w == 0) atomicAdd(s.err, 1ull);
            return;
        }
        reinterpret_cast<uint4 *>(b.envs)[(size_t)i * W + w] = reinterpret_cast<const uint4 *>(s.env)[(size_t)e * W + w];
        return;
    }
    const uint32_t g = (blockIdx.x - nb_env) * kSnapBlock + threadIdx.x;
    if (g >= (uint32_t)rec.cap * (uint32_t)b.N) return;
    const uint32_t slot = g / (uint32_t)b.N, i = g - slot * (uint32_t)b.N;
    const int e = src ? src[i] : ((int)i < s.n ? (int)i : -1);
    if (e < 0 || !entry_fits(s, e, (int)i, b.n_inst)) return;
    rec.rec[g] = s.rec[(size_t)slot * (uint32_t)s.n + (uint32_t)e];
}

uint32_t blocks(size_t n) { return (uint32_t)((n + kSnapBlock - 1) / kSnapBlock); }

}  // namespace

int launch_snapshot_save(const DevBatch &b, const SchedRec &rec, const SnapBuf &s, const int32_t *idx, hipStream_t st) {
    const size_t W = b.L.e_stride / 16u;
    const uint32_t nb_env = blocks((size_t)s.n * W);
    const uint32_t nb_rec = (rec.rec && s.cap > 0) ? blocks((size_t)s.cap * (size_t)s.n) : 0u;
    SchedRec r = rec;
    SnapBuf sb = s;
    if (!nb_rec) sb.cap = 0;
    hipLaunchKernelGGL(snapshot_save_kernel, dim3(nb_env + nb_rec), dim3(kSnapBlock), 0, st, b, r, sb, idx, nb_env);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_snapshot_load(const DevBatch &b, const SchedRec &rec, const SnapBuf &s, const int32_t *src, hipStream_t st) {
    const size_t W = b.L.e_stride / 16u;
    const uint32_t nb_env = blocks((size_t)b.N * W);
    const uint32_t nb_rec = (rec.rec && s.cap > 0) ? blocks((size_t)rec.cap * (size_t)b.N) : 0u;
    SchedRec r = rec;
    if (!nb_rec) r.cap = 0;
    hipLaunchKernelGGL(snapshot_load_kernel, dim3(nb_env + nb_rec), dim3(kSnapBlock), 0, st, b, r, s, src, nb_env);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace fjsp
