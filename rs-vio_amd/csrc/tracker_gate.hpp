// tracker_gate.hpp -- the stereo gate: an epipolar check on the pairs of a frame, in the frame-end
// workgroup.  Part of tracker.hip's translation unit (it uses block_exclusive_scan and runs inside
// append_pack, between the append of the new points and the packing loop).
//
// The contract is include/rsvio_gpu.h's (rsvio_tracker_set_stereo_gate).  For every id present in
// both cameras' maps: the bearings from the stored f32 unprojected coordinates promoted to f64,
// e = |d_l . (E d_r)| with E = [t / |t|]x R from the host, rejected when invalid or !(e <= max_error).
// gate_flags() is the join and the decision (also the whole of the stateless entry
// rsvio_stereo_gate_lists); gate_compact() applies it to the track maps as remove_ids_kernel does.
// Both walk ceil(n / blockDim.x) consecutive entries per thread, so the lists may be longer than
// the block.
#pragma once

// What the frame-end workgroup needs for one handle's gate (by value in the single launch, in the
// BatchSlot of the batched one)
struct GateDev {
    int mode;            // RSVIO_GATE_*; OFF: append_pack does nothing more than without a gate
    int reserved;
    double max_error;
    double E[9];         // row-major
    uint8_t* keep;       // scratch: 2 x capacity keep flags (cam0, cam1)
    double* err;         // scratch: capacity, e of every cam1 entry
    float* tmp_aff;      // scratch: 2 x capacity x 6 (the gate's own: append_pack reads the handle's through
                         // __restrict__ pointers)
    float2* tmp_und;     // scratch: capacity
    uint64_t* rep_ids;   // the frame's report, in its output slot: rejected ids ascending ...
    double* rep_err;     // ... and their e (NaN: invalid)
    int* counters;       // {n_pairs, n_rejected, n_invalid, 0}, read back with the frame's counts
};

// A bearing from stored coordinates; false: invalid (a NaN coordinate, or RAY with s < 0)
__device__ __forceinline__ bool gate_bearing(int convention, float2 uv, double d[3]) {
    const double x = (double)uv.x, y = (double)uv.y;
    if (x != x || y != y) return false;
    if (convention == RSVIO_UNPROJ_RAY) {
        const double s = (1.0 - x * x) - y * y;
        if (s < 0.0) return false;
        d[0] = x;
        d[1] = y;
        d[2] = sqrt(s);
    } else {
        const double n = sqrt((x * x + y * y) + 1.0);
        d[0] = x / n;
        d[1] = y / n;
        d[2] = 1.0 / n;
    }
    return true;
}

// The join and the decision, one workgroup.  ids0 / ids1 ascending; keep0[n0], keep1[n1], err1[n1]
// are written for every entry (keep 1 and e = NaN for an unpaired cam1 entry); cnt (LDS, 3 ints)
// gets {pairs, rejected, invalid}.  Ends with a barrier: flags and counters are visible to the block.
__device__ __forceinline__ void gate_flags(int mode, double max_error, const double* E, int conv0, int conv1,
                                           const uint64_t* __restrict__ ids0, const float2* __restrict__ und0, int n0,
                                           const uint64_t* __restrict__ ids1, const float2* __restrict__ und1, int n1,
                                           uint8_t* __restrict__ keep0, uint8_t* __restrict__ keep1,
                                           double* __restrict__ err1, int* cnt) {
    const int tid = threadIdx.x;
    if (tid < 3) cnt[tid] = 0;
    for (int i = tid; i < n0; i += blockDim.x) keep0[i] = 1;
    __syncthreads();
    const int per = (n1 + blockDim.x - 1) / blockDim.x;
    const int b = min(n1, tid * per), e = min(n1, b + per);
    int pairs = 0, rejected = 0, invalid = 0;
    for (int j = b; j < e; ++j) {
        const uint64_t id = ids1[j];
        int lo = 0, hi = n0;  // first i with ids0[i] >= id
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ids0[mid] < id) lo = mid + 1; else hi = mid;
        }
        double err = __builtin_nan("");
        bool rej = false;
        if (lo < n0 && ids0[lo] == id) {
            ++pairs;
            double dl[3], dr[3];
            const bool ok_l = gate_bearing(conv0, und0[lo], dl);
            const bool ok_r = gate_bearing(conv1, und1[j], dr);
            if (ok_l && ok_r) {
                const double v0 = E[0] * dr[0] + E[1] * dr[1] + E[2] * dr[2];
                const double v1 = E[3] * dr[0] + E[4] * dr[1] + E[5] * dr[2];
                const double v2 = E[6] * dr[0] + E[7] * dr[1] + E[8] * dr[2];
                err = fabs(dl[0] * v0 + dl[1] * v1 + dl[2] * v2);
                rej = !(err <= max_error);
            } else {
                ++invalid;
                rej = true;
            }
            if (rej) {
                ++rejected;
                if (mode == RSVIO_GATE_DROP_BOTH) keep0[lo] = 0;  // (ids are unique: one writer per entry)
            }
        }
        keep1[j] = rej ? 0 : 1;
        err1[j] = err;
    }
    if (pairs) atomicAdd(&cnt[0], pairs);
    if (rejected) atomicAdd(&cnt[1], rejected);
    if (invalid) atomicAdd(&cnt[2], invalid);
    __syncthreads();
}

// The flags applied to one camera's map: ids, affines and stored coordinates compacted in order
// through the temporaries; for cam1 (report = true) the dropped entries, which are the rejected ones,
// go to the report in order.  Returns the new length.  Ends with a barrier.
__device__ __forceinline__ int gate_compact(const GateDev& g, int c, int n, int capacity, uint64_t* __restrict__ ids,
                                            float* __restrict__ ma, float2* __restrict__ und,
                                            uint64_t* __restrict__ ids_tmp, int* sh) {
    const int tid = threadIdx.x;
    const uint8_t* keep = g.keep + (size_t)c * capacity;
    uint64_t* it = ids_tmp + (size_t)c * capacity;
    float* ta = g.tmp_aff + (size_t)c * capacity * 6;
    const int per = (n + blockDim.x - 1) / blockDim.x;
    const int b = min(n, tid * per), e = min(n, b + per);
    int local = 0;
    for (int i = b; i < e; ++i) {
        local += keep[i] ? 1 : 0;
        it[i] = ids[i];
        for (int k = 0; k < 6; ++k) ta[6 * i + k] = ma[6 * i + k];
        g.tmp_und[i] = und[i];
    }
    int total;
    int pos = block_exclusive_scan(local, sh, &total);  // its barriers order the copies
    for (int i = b; i < e; ++i) {
        if (keep[i]) {
            ids[pos] = it[i];
            for (int k = 0; k < 6; ++k) ma[6 * pos + k] = ta[6 * i + k];
            und[pos] = g.tmp_und[i];
            ++pos;
        } else if (c == 1) {
            g.rep_ids[i - pos] = it[i];
            g.rep_err[i - pos] = g.err[i];
        }
    }
    __syncthreads();
    return total;
}

// The gate at the end of a frame: both maps hold m0 / m1 entries with their stored coordinates in
// und0 / und1 (map order).  Updates m0, m1 and writes the counters.
__device__ __forceinline__ void stereo_gate(const GateDev& g, int conv0, int conv1, int capacity,
                                            uint64_t* __restrict__ ids0, uint64_t* __restrict__ ids1,
                                            float* __restrict__ map_aff0, float* __restrict__ map_aff1,
                                            float2* __restrict__ und0, float2* __restrict__ und1,
                                            uint64_t* __restrict__ ids_tmp, int* sh, int& m0, int& m1) {
    __shared__ int cnt[3];
    gate_flags(g.mode, g.max_error, g.E, conv0, conv1, ids0, und0, m0, ids1, und1, m1, g.keep, g.keep + capacity,
               g.err, cnt);
    const int pairs = cnt[0], rejected = cnt[1], invalid = cnt[2];
    if (rejected) {  // (block-uniform)
        m1 = gate_compact(g, 1, m1, capacity, ids1, map_aff1, und1, ids_tmp, sh);
        if (g.mode == RSVIO_GATE_DROP_BOTH) m0 = gate_compact(g, 0, m0, capacity, ids0, map_aff0, und0, ids_tmp, sh);
    }
    if (threadIdx.x == 0) {
        g.counters[0] = pairs;
        g.counters[1] = rejected;
        g.counters[2] = invalid;
        g.counters[3] = 0;
    }
}

// rsvio_dbg_stereo_gate_frame (diagnostic): the frame end's whole gate -- flags, compaction, report
// -- on two given maps, so that maps longer than the block can be tested (no frame reaches them)
__global__ __launch_bounds__(1024) void stereo_gate_frame_kernel(GateDev g, int conv0, int conv1, int capacity,
                                                                 uint64_t* ids0, uint64_t* ids1, float* aff0, float* aff1,
                                                                 float2* und0, float2* und1, uint64_t* ids_tmp, int n0,
                                                                 int n1, int* __restrict__ out_n) {
    __shared__ int sh[1024];
    int m0 = n0, m1 = n1;
    stereo_gate(g, conv0, conv1, capacity, ids0, ids1, aff0, aff1, und0, und1, ids_tmp, sh, m0, m1);
    if (threadIdx.x == 0) {
        out_n[0] = m0;
        out_n[1] = m1;
    }
}

// rsvio_stereo_gate_lists: gate_flags alone, on two lists in device memory
__global__ __launch_bounds__(1024) void stereo_gate_lists_kernel(
    int mode, double max_error, const double* __restrict__ E, int conv0, int conv1, const uint64_t* __restrict__ ids0,
    const float2* __restrict__ und0, int n0, const uint64_t* __restrict__ ids1, const float2* __restrict__ und1, int n1,
    uint8_t* __restrict__ keep0, uint8_t* __restrict__ keep1, double* __restrict__ err1, int* __restrict__ counters) {
    __shared__ int cnt[3];
    __shared__ double Es[9];
    if (threadIdx.x < 9) Es[threadIdx.x] = E[threadIdx.x];
    __syncthreads();
    gate_flags(mode, max_error, Es, conv0, conv1, ids0, und0, n0, ids1, und1, n1, keep0, keep1, err1, cnt);
    if (threadIdx.x < 3) counters[threadIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x == 3) counters[3] = 0;
}
