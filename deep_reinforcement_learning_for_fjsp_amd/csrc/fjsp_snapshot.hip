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

#include <cstring>
#include <string>

#include "fjsp_env_impl.h"

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

// ---- host side: the fjsp_snapshot_* ABI

using namespace fjsp;

namespace {
// what two batches must share for a snapshot of one to be loaded into the other (N may differ)
struct SnapFingerprint {
    Layout L;
    int32_t KC, KP, MP, JP, variant, n_obs, n_static, mord, single_job, grp, n_inst, pad;
    uint64_t inst_hash;
};

SnapFingerprint fingerprint_of(const fjsp_env *e) {
    SnapFingerprint f;
    std::memset(&f, 0, sizeof(f));
    const DevBatch &b = e->b;
    f.L = b.L;
    f.KC = b.KC; f.KP = b.KP; f.MP = b.MP; f.JP = b.JP; f.variant = b.variant; f.n_obs = b.n_obs; f.n_static = b.n_static;
    f.mord = b.mord; f.single_job = b.single_job; f.grp = b.grp; f.n_inst = b.n_inst;
    f.inst_hash = e->inst_hash;
    return f;
}

// serialised form (fjsp_snapshot_to_host): this header, the fingerprint, then the device buffer as it is
struct SnapBlobHeader {
    char magic[8];
    uint32_t version, fp_bytes;
    int32_t n, cap, rec_valid, pad;
    uint64_t buf_bytes;
};
constexpr char kSnapMagic[8] = {'F', 'J', 'S', 'P', 'S', 'N', 'A', 'P'};

size_t snap_hdr_off(int32_t n, uint32_t e_stride) { return (size_t)n * e_stride; }
size_t snap_rec_off(int32_t n, uint32_t e_stride) { return snap_hdr_off(n, e_stride) + ((size_t)n * 8 + 15) / 16 * 16; }
size_t snap_bytes(int32_t n, int32_t cap, uint32_t e_stride) { return snap_rec_off(n, e_stride) + (size_t)cap * (size_t)n * 16; }

int same_fingerprint(const fjsp_env *e, const SnapFingerprint &fp, const char *who) {
    const SnapFingerprint mine = fingerprint_of(e);
    if (std::memcmp(&fp, &mine, sizeof(fp)) == 0) return FJSP_OK;
    set_error(std::string(who) + ": the batch is not compatible with the snapshot (other instances, variant, kernel family or record layout)");
    return FJSP_E_ARG;
}
}  // namespace

struct fjsp_snapshot {
    int device = 0;
    SnapFingerprint fp{};
    int32_t n = 0, cap = 0;            // entries; record slots per entry (0: the buffer holds no dispatch records)
    bool rec_valid = false;            // the last save came from a recording batch (the record area holds its records)
    unsigned char *buf = nullptr;
    size_t bytes = 0;
    unsigned long long *d_err = nullptr;
    SnapBuf view() const {
        SnapBuf v;
        v.env = buf;
        v.hdr = reinterpret_cast<int2 *>(buf + snap_hdr_off(n, fp.L.e_stride));
        v.rec = cap > 0 ? reinterpret_cast<uint4 *>(buf + snap_rec_off(n, fp.L.e_stride)) : nullptr;
        v.err = d_err;
        v.n = n; v.cap = cap;
        return v;
    }
};

static int snapshot_alloc(int device, const SnapFingerprint &fp, int32_t n, int32_t cap, fjsp_snapshot **out) {
    if ((size_t)n * (fp.L.e_stride / 16) >= ((size_t)1 << 32) || (size_t)n * (size_t)cap >= ((size_t)1 << 32)) {
        set_error("fjsp_snapshot_create: snapshot too large (n x record size / 16 and n x cap must stay below 2^32)");
        return FJSP_E_UNSUPPORTED;
    }
    auto *s = new fjsp_snapshot();
    s->device = device; s->fp = fp; s->n = n; s->cap = cap;
    s->bytes = snap_bytes(n, cap, fp.L.e_stride);
    const size_t hoff = snap_hdr_off(n, fp.L.e_stride);
    if (!hip_ok(hipMalloc(&s->buf, s->bytes), "hipMalloc snapshot") ||
        !hip_ok(hipMalloc(&s->d_err, 16), "hipMalloc snapshot error counter") ||
        !hip_ok(hipMemset(s->d_err, 0, 16), "hipMemset") ||
        !hip_ok(hipMemset(s->buf + hoff, 0xFF, (size_t)n * 8), "hipMemset")) {        // headers {-1, -1}: nothing saved yet
        fjsp_snapshot_destroy(s);
        return FJSP_E_HIP;
    }
    *out = s;
    return FJSP_OK;
}

static int snapshot_usable(const fjsp_snapshot *s, const fjsp_env *e, const char *who) {
    if (!s || !e) { set_error(std::string(who) + ": null argument"); return FJSP_E_ARG; }
    if (const int rc = usable(e, who, kIntact | kIdle)) return rc;
    if (s->device != e->device) { set_error(std::string(who) + ": the snapshot lives on another device than the batch"); return FJSP_E_ARG; }
    return same_fingerprint(e, s->fp, who);
}

extern "C" {
int fjsp_snapshot_create(const fjsp_env *e, int32_t n, fjsp_snapshot **out) {
    if (!e || !out || n <= 0) { set_error("fjsp_snapshot_create: bad arguments"); return FJSP_E_ARG; }
    DeviceGuard guard(e->device);
    return snapshot_alloc(e->device, fingerprint_of(e), n, e->sched.rec ? e->sched.cap : 0, out);
}

void fjsp_snapshot_destroy(fjsp_snapshot *s) {
    if (!s) return;
    {
        DeviceGuard guard(s->device);
        if (s->buf) (void)hipFree(s->buf);
        if (s->d_err) (void)hipFree(s->d_err);
    }
    delete s;
}

int fjsp_snapshot_size(const fjsp_snapshot *s) { return s ? s->n : 0; }
int fjsp_snapshot_capacity(const fjsp_snapshot *s) { return s ? s->cap : 0; }

int fjsp_snapshot_save(fjsp_snapshot *s, fjsp_env *e, const int32_t *d_idx, void *stream) {
    if (const int rc = snapshot_usable(s, e, "fjsp_snapshot_save")) return rc;
    if (!d_idx && s->n > e->b.N) { set_error("fjsp_snapshot_save: the snapshot has more entries than the batch has envs (pass d_idx)"); return FJSP_E_ARG; }
    const bool with_rec = s->cap > 0 && e->sched.rec != nullptr;
    if (with_rec && e->sched.cap != s->cap) { set_error("fjsp_snapshot_save: record capacity differs from the batch's"); return FJSP_E_STATE; }
    DeviceGuard guard(e->device);
    if (launch_snapshot_save(e->b, with_rec ? e->sched : SchedRec{}, s->view(), d_idx, (hipStream_t)stream) != 0) {
        set_error("snapshot_save_kernel launch failed"); return FJSP_E_HIP;
    }
    s->rec_valid = with_rec;
    return FJSP_OK;
}

int fjsp_snapshot_load(fjsp_snapshot *s, fjsp_env *e, const int32_t *d_src, void *stream) {
    if (const int rc = snapshot_usable(s, e, "fjsp_snapshot_load")) return rc;
    if (e->sched.rec && (!s->rec_valid || s->cap != e->sched.cap)) {
        set_error("fjsp_snapshot_load: the batch records its schedule but the snapshot holds no dispatch records (save it from a recording batch)");
        return FJSP_E_STATE;
    }
    if ((size_t)e->b.N * (e->b.L.e_stride / 16) >= ((size_t)1 << 32) || (size_t)e->b.N * (size_t)e->sched.cap >= ((size_t)1 << 32)) {
        set_error("fjsp_snapshot_load: batch too large for the copy kernel's 32-bit indices"); return FJSP_E_UNSUPPORTED;
    }
    DeviceGuard guard(e->device);
    if (launch_snapshot_load(e->b, e->sched.rec ? e->sched : SchedRec{}, s->view(), d_src, (hipStream_t)stream) != 0) {
        set_error("snapshot_load_kernel launch failed"); return FJSP_E_HIP;
    }
    return FJSP_OK;
}

int fjsp_snapshot_errors(fjsp_snapshot *s, int64_t *count) {
    if (!s || !count) { set_error("fjsp_snapshot_errors: null argument"); return FJSP_E_ARG; }
    DeviceGuard guard(s->device);
    unsigned long long v = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&v, s->d_err, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(s->d_err, 0, 8));
    *count = (int64_t)v;
    return FJSP_OK;
}

int fjsp_snapshot_to_host(fjsp_snapshot *s, void *h_out, int64_t *nbytes) {
    if (!s || !nbytes) { set_error("fjsp_snapshot_to_host: null argument"); return FJSP_E_ARG; }
    const size_t need = sizeof(SnapBlobHeader) + sizeof(SnapFingerprint) + s->bytes;
    if (!h_out) { *nbytes = (int64_t)need; return FJSP_OK; }
    if (*nbytes < (int64_t)need) { set_error("fjsp_snapshot_to_host: output buffer too small"); return FJSP_E_ARG; }
    SnapBlobHeader h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, kSnapMagic, 8);
    h.version = 1; h.fp_bytes = (uint32_t)sizeof(SnapFingerprint);
    h.n = s->n; h.cap = s->cap; h.rec_valid = s->rec_valid ? 1 : 0; h.buf_bytes = s->bytes;
    unsigned char *o = static_cast<unsigned char *>(h_out);
    std::memcpy(o, &h, sizeof(h));
    std::memcpy(o + sizeof(h), &s->fp, sizeof(SnapFingerprint));
    DeviceGuard guard(s->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(o + sizeof(h) + sizeof(SnapFingerprint), s->buf, s->bytes, hipMemcpyDeviceToHost));
    *nbytes = (int64_t)need;
    return FJSP_OK;
}

int fjsp_snapshot_from_host(const fjsp_env *e, const void *h_in, int64_t nbytes, fjsp_snapshot **out) {
    if (!e || !h_in || !out || nbytes < (int64_t)(sizeof(SnapBlobHeader) + sizeof(SnapFingerprint))) {
        set_error("fjsp_snapshot_from_host: bad arguments"); return FJSP_E_ARG;
    }
    SnapBlobHeader h;
    const unsigned char *p = static_cast<const unsigned char *>(h_in);
    std::memcpy(&h, p, sizeof(h));
    if (std::memcmp(h.magic, kSnapMagic, 8) != 0 || h.version != 1 || h.fp_bytes != sizeof(SnapFingerprint)) {
        set_error("fjsp_snapshot_from_host: not a snapshot of this library version"); return FJSP_E_ARG;
    }
    SnapFingerprint fp;
    std::memcpy(&fp, p + sizeof(h), sizeof(fp));
    if (const int rc = same_fingerprint(e, fp, "fjsp_snapshot_from_host")) return rc;
    if (h.n <= 0 || h.cap < 0 || h.buf_bytes != snap_bytes(h.n, h.cap, fp.L.e_stride) ||
        (uint64_t)nbytes != sizeof(h) + sizeof(fp) + h.buf_bytes) {
        set_error("fjsp_snapshot_from_host: truncated or inconsistent snapshot bytes"); return FJSP_E_ARG;
    }
    DeviceGuard guard(e->device);
    fjsp_snapshot *s = nullptr;
    int rc = snapshot_alloc(e->device, fp, h.n, h.cap, &s);
    if (rc != FJSP_OK) return rc;
    if (!hip_ok(hipMemcpy(s->buf, p + sizeof(h) + sizeof(fp), s->bytes, hipMemcpyHostToDevice), "upload snapshot")) {
        fjsp_snapshot_destroy(s); return FJSP_E_HIP;
    }
    s->rec_valid = h.rec_valid != 0;
    *out = s;
    return FJSP_OK;
}
}  // extern "C"
