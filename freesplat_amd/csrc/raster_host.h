// raster_host.h -- host-only facts of the rasterizer that raster_fwd.hip and raster_bwd.hip share: the byte layouts of the
// opaque per-view buffers (each offset is computed here and nowhere else) and the fork/join event set of the views drivers.
#pragma once
#include "fs_common.h"

namespace fs {

template <typename T>
inline T* at(const void* base, size_t offset) { return (T*)((char*)base + offset); }

// binning: [T+1] u32 tile ranges (exclusive scan of the per-tile counts) | [cap] u32 point list
struct BinningLayout {
    size_t point_list, total;
    BinningLayout(int H, int W, long long cap = 1)
        : point_list(binning_offsets_bytes(H, W)), total(point_list + align_up((size_t)(cap > 0 ? cap : 1) * 4, 256)) {}
    // list entries a buffer of `bytes` holds past the tile ranges (0: too small) -- how a views call reads its instance
    // capacity back from the binning stride
    static size_t capacity(int H, int W, size_t bytes)
    {
        const size_t ranges = binning_offsets_bytes(H, W);
        return bytes > ranges ? (bytes - ranges) / 4 : 0;
    }
};

// image: [P] f32 final_T | [P] i32 n_contrib
struct ImageLayout {
    size_t n_contrib, total;
    ImageLayout(int H, int W) : n_contrib(align_up((size_t)H * W * 4, 256)), total(2 * n_contrib) {}
};

// forward scratch: [T] u32 tile counts | [T x tile_cap] u64 key areas (tile_capacity, fs_common.h)
struct FwdScratchLayout {
    int T;
    uint32_t tile_cap;
    size_t keys, total;
    FwdScratchLayout(int H, int W, long long cap)
        : T(num_tiles(H, W)), tile_cap(tile_capacity(cap, T)), keys(align_up((size_t)T * 4, 256)),
          total(keys + align_up((size_t)T * tile_cap * 8, 256)) {}
};

// backward scratch: the [N, 12] f32 gradient rows of every view, 256-byte aligned | with FS_RASTER_DETERMINISTIC one region
// (raster_bwd.hip DetRegion, `region_bytes` each) per stream in flight.  v = 0 is the single-view form: one view, and without
// regions the rows unpadded.
struct BwdScratchLayout {
    size_t row_stride, regions, region_bytes, total;
    BwdScratchLayout(int N, int v, int n_regions, size_t region_bytes_)
        : row_stride(align_up((size_t)N * 48, 256)), regions((size_t)(v > 0 ? v : 1) * row_stride), region_bytes(region_bytes_),
          total(n_regions > 0 ? regions + (size_t)n_regions * region_bytes : (v == 0 ? (size_t)N * 48 : regions)) {}
    size_t rows(int view) const { return row_stride * view; }
    size_t region(int k) const { return regions + region_bytes * k; }
};

// ---- side streams of a views call ----------------------------------------------------------------------------------
constexpr int kMaxStreams = 8;          // side streams a views call may use
constexpr int kMaxViewsInFlight = 16;   // key areas (scratch slots) a multi-view call may use at once

// Cached events: fork `main` into the side streams (the forward forks per batch of views: record + one wait per view), join
// them back.  Events belong to the device that was current when they
// were created: one set per (thread, device), made on the first call that uses side streams and kept.
struct ForkJoin {
    hipEvent_t ready = nullptr, done[kMaxStreams] = {}, batch[kMaxViewsInFlight] = {};
    bool ok = false;
    ForkJoin()
    {
        ok = hipEventCreateWithFlags(&ready, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < kMaxStreams && ok; ++i) ok = hipEventCreateWithFlags(&done[i], hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < kMaxViewsInFlight && ok; ++i) ok = hipEventCreateWithFlags(&batch[i], hipEventDisableTiming) == hipSuccess;
    }
    static ForkJoin* get()   // nullptr (last error set) when the device or the events cannot be had
    {
        static thread_local ForkJoin* per_device[64] = {};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { set_last_error("hipGetDevice", hipGetLastError()); return nullptr; }
        if (!per_device[dev]) per_device[dev] = new ForkJoin();
        if (!per_device[dev]->ok) { set_last_error("event create", hipGetLastError()); return nullptr; }
        return per_device[dev];
    }
    static int record(hipEvent_t e, hipStream_t on, const char* what = "event record")
    {
        if (hipEventRecord(e, on) == hipSuccess) return FS_OK;
        set_last_error(what, hipGetLastError());
        return FS_ERR_LAUNCH;
    }
    static int wait(hipStream_t st, hipEvent_t e, const char* what = "stream wait")
    {
        if (hipStreamWaitEvent(st, e, 0) == hipSuccess) return FS_OK;
        set_last_error(what, hipGetLastError());
        return FS_ERR_LAUNCH;
    }
    int fork(hipStream_t main, void* const* streams, int ns)   // the side streams wait for what is queued on main now
    {
        int rc = record(ready, main);
        for (int s = 0; s < ns && rc == FS_OK; ++s) rc = wait((hipStream_t)streams[s], ready);
        return rc;
    }
    int join(hipStream_t main, void* const* streams, int ns)   // main waits for everything queued on the side streams
    {
        int rc = FS_OK;
        for (int s = 0; s < ns && rc == FS_OK; ++s) {
            rc = record(done[s], (hipStream_t)streams[s], "stream join");
            if (rc == FS_OK) rc = wait(main, done[s], "stream join");
        }
        return rc;
    }
};

}  // namespace fs
