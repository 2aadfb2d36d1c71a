// tracker_batch.hpp -- batched process_frame: one stereo frame per tracker handle, n handles per
// call (the serving mode's tracker leg beside rsvio_ba_batch_* and rsvio_pnp_batch_*).  Part of
// tracker.hip's translation unit (it works on rsvio::Tracker's state and reuses append_pack).
//
// One call, on the batch's own stream:
//   upload   ONE copy: the descriptor tables and the staged host images
//   K1 + K3  ONE pyramid launch over 2n images, per-image source / pyramid / FAST outputs from a
//            device table (pyramid.hpp PyrSlot); FAST-9 cells on every left image
//   K2       ONE table-mode LK launch of up to 3n batches (cam0 and cam1 temporal of the streams
//            with history, every stream's stereo cell jobs with its cell mask)
//   Ka       ONE launch, workgroup i = stream i: append_pack with its arguments from a device
//            descriptor, then the lists gathered into the batch's read-back buffer
//   download ONE copy, ONE host wait
// Each handle's buffers are the ones its own process_frame would use (pyramid ping-pong slot, track
// maps, output slot), and the host state is advanced as submit + fetch advance it, so the results
// are the single call's byte for byte and both kinds of call may alternate on a handle.
#pragma once

namespace rsvio {

namespace {

// append_pack's arguments for one stream, and where its lists go in the read-back buffer
struct BatchSlot {
    int* bins;
    int n0, n1, tracked, capacity;
    const float* at0;
    const float* at1;
    const uint8_t* tv0;
    const uint8_t* tv1;
    uint64_t* ids_tmp;
    const int4* cell_pt;
    const float* new_aff0;
    const float* new_aff1;
    const uint8_t* new_valid;
    float* map_aff0;
    float* map_aff1;
    uint64_t* ids0;
    uint64_t* ids1;
    int* counts;
    unsigned long long* last_id;
    rsvio_feature* out0;
    rsvio_feature* out1;
    int* overflow;
    float2* und0;
    float2* und1;
    int* rb_head;          // {n_l, n_r, overflow, 0, gate: n_pairs, n_rejected, n_invalid, 0}
    rsvio_feature* rb[2];  // bnd[c] entries each
    float2* rbu[2];        // likewise, with cameras
    int bnd[2];            // the host-known bound of each list (submit's)
    CamPair cams;
    GateDev gate;          // the handle's stereo gate (mode OFF: none); read by the gate launch only
};

__global__ __launch_bounds__(1024) void append_pack_batch_kernel(GridGeom G, int n_cells,
                                                                 const BatchSlot* __restrict__ slots) {
    const BatchSlot& d = slots[blockIdx.x];
    append_pack<false>(G, d.bins, d.n0, d.n1, d.tracked, d.at0, d.at1, d.tv0, d.tv1, d.ids_tmp, d.cell_pt, n_cells,
                       d.new_aff0, d.new_aff1, d.new_valid, d.map_aff0, d.map_aff1, d.ids0, d.ids1, d.counts,
                       d.last_id, d.capacity, d.out0, d.out1, d.overflow, d.cams, d.und0, d.und1, GateDev{});
    __syncthreads();  // the lists and counts are this workgroup's own writes
    const int m0 = d.counts[0], m1 = d.counts[1];
    if (threadIdx.x == 0) {
        d.rb_head[0] = m0;
        d.rb_head[1] = m1;
        d.rb_head[2] = *d.overflow;
        d.rb_head[3] = 0;
    }
    const int k0 = min(m0, d.bnd[0]), k1 = min(m1, d.bnd[1]);
    for (int j = threadIdx.x; j < k0 + k1; j += blockDim.x) {
        const int c = j < k0 ? 0 : 1;
        const int i = c == 0 ? j : j - k0;
        d.rb[c][i] = (c == 0 ? d.out0 : d.out1)[i];
        if (d.cams.on) d.rbu[c][i] = (c == 0 ? d.und0 : d.und1)[i];
    }
}

// The same launch when some handle of the batch has a stereo gate set: each workgroup follows its
// own slot's gate, and the gate's counters join the head.  (A launch of its own, not a template
// over the one above: that one stays the code it was, instruction for instruction.)
__global__ __launch_bounds__(1024) void append_pack_batch_gate_kernel(GridGeom G, int n_cells,
                                                                      const BatchSlot* __restrict__ slots) {
    const BatchSlot& d = slots[blockIdx.x];
    append_pack<true>(G, d.bins, d.n0, d.n1, d.tracked, d.at0, d.at1, d.tv0, d.tv1, d.ids_tmp, d.cell_pt, n_cells,
                      d.new_aff0, d.new_aff1, d.new_valid, d.map_aff0, d.map_aff1, d.ids0, d.ids1, d.counts,
                      d.last_id, d.capacity, d.out0, d.out1, d.overflow, d.cams, d.und0, d.und1, d.gate);
    __syncthreads();
    const int m0 = d.counts[0], m1 = d.counts[1];
    if (threadIdx.x == 0) {
        d.rb_head[0] = m0;
        d.rb_head[1] = m1;
        d.rb_head[2] = *d.overflow;
        d.rb_head[3] = 0;
    }
    if (threadIdx.x < 4) d.rb_head[4 + threadIdx.x] = d.gate.mode != RSVIO_GATE_OFF ? d.gate.counters[threadIdx.x] : 0;
    const int k0 = min(m0, d.bnd[0]), k1 = min(m1, d.bnd[1]);
    for (int j = threadIdx.x; j < k0 + k1; j += blockDim.x) {
        const int c = j < k0 ? 0 : 1;
        const int i = c == 0 ? j : j - k0;
        d.rb[c][i] = (c == 0 ? d.out0 : d.out1)[i];
        if (d.cams.on) d.rbu[c][i] = (c == 0 ? d.und0 : d.und1)[i];
    }
}

inline size_t up32(size_t v) { return (v + 31) & ~(size_t)31; }

bool same_params(const rsvio_tracker_params& a, const rsvio_tracker_params& b) {
    return a.width == b.width && a.height == b.height && a.levels == b.levels && a.grid_size == b.grid_size &&
           a.max_iterations == b.max_iterations &&
           std::memcmp(&a.convergence_threshold, &b.convergence_threshold, sizeof(float)) == 0 &&
           a.device == b.device && a.max_features == b.max_features;
}

}  // namespace

struct TrackerBatch {
    int n = 0;
    std::vector<Tracker*> T;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // upload: [PyrSlot 2n][rsvio_track_batch 3n][mask pointer 3n][BatchSlot n][tstart 3n + 1][images]
    size_t off_pyr = 0, off_lk = 0, off_mask = 0, off_slot = 0, off_start = 0, off_img = 0, img_stride = 0;
    HostBuf<uint8_t> h_up;
    DevBuf<uint8_t> d_up;
    // read-back: per stream a 32-B head, both lists and (with cameras) both undistorted lists
    HostBuf<uint8_t> h_rb;
    DevBuf<uint8_t> d_rb;
    std::vector<size_t> rb_off;  // per stream: head, list 0, list 1, undistorted 0, undistorted 1
    std::vector<size_t> bnd;     // per stream and camera: the host-known bound of the list (submit's)

    void init(rsvio_tracker* const* handles, int n_) {
        n = n_;
        T.resize(n);
        for (int i = 0; i < n; ++i) T[i] = &handles[i]->t;
        const Tracker& t0 = *T[0];
        RSVIO_HIP(hipSetDevice(t0.P.device));
        RSVIO_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        RSVIO_HIP(hipEventCreate(&ev[0]));
        RSVIO_HIP(hipEventCreate(&ev[1]));
        size_t o = 0;
        off_pyr = o;   o = up32(o + sizeof(PyrSlot) * 2 * n);
        off_lk = o;    o = up32(o + sizeof(rsvio_track_batch) * 3 * n);
        off_mask = o;  o = up32(o + sizeof(const int4*) * 3 * n);
        off_slot = o;  o = up32(o + sizeof(BatchSlot) * n);
        off_start = o; o = up32(o + sizeof(int32_t) * (3 * n + 1));
        off_img = o;
        img_stride = up32((size_t)t0.P.width * t0.P.height);
        rb_off.resize((size_t)5 * n);
        bnd.resize((size_t)2 * n);
        grow_upload(0);
    }
    ~TrackerBatch() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }

    void grow_upload(size_t n_host_images) {
        const size_t need = off_img + n_host_images * img_stride;
        if (h_up.n >= need && h_up.n) return;
        h_up.alloc(std::max(need, (size_t)32));
        d_up.alloc(std::max(need, (size_t)32));
    }

    template <class U>
    U* hp(size_t off) { return reinterpret_cast<U*>(h_up.p + off); }
    template <class U>
    U* dp(size_t off) { return reinterpret_cast<U*>(d_up.p + off); }

    // Every argument check of a call, before anything is launched or written
    void validate(const rsvio_stereo_frame* f) const {
        const size_t w = (size_t)T[0]->P.width;
        for (int i = 0; i < n; ++i) {
            const std::string at = "rsvio_tracker_batch_process_frames: slot " + std::to_string(i) + ": ";
            if (!f[i].left || !f[i].right) throw std::invalid_argument(at + "NULL image");
            if (f[i].on_device != 0 && f[i].on_device != 1) throw std::invalid_argument(at + "on_device must be 0 or 1");
            if (f[i].on_device ? (f[i].stride != 0 && f[i].stride != w) : (f[i].stride != 0 && f[i].stride < w))
                throw std::invalid_argument(at + (f[i].on_device ? "device images are tightly packed (stride 0 or width)"
                                                                 : "stride < width"));
            if ((f[i].cap_l && !f[i].out_l) || (f[i].cap_r && !f[i].out_r))
                throw std::invalid_argument(at + "NULL list with a capacity");
            if (T[i]->inflight) throw CallOrderError(at + "a frame is in flight on this handle (collect it first)");
            // (the batched launch tracks every feature from its own position: the prediction stays pending)
            if (T[i]->pred_pending)
                throw std::invalid_argument(at + "a prediction is pending on this handle (rsvio_tracker_set_prediction; "
                                                 "the batched call does not seed)");
        }
    }

    int run(rsvio_stereo_frame* f, double* device_ms) {
        validate(f);
        const Tracker& t0 = *T[0];
        const size_t w = (size_t)t0.P.width, h = (size_t)t0.P.height;
        RSVIO_HIP(hipSetDevice(t0.P.device));
        size_t n_host = 0;
        for (int i = 0; i < n; ++i) n_host += f[i].on_device ? 0 : 2;
        grow_upload(n_host);
        // the read-back layout, from each stream's host-known list bounds
        size_t rb = 0;
        for (int i = 0; i < n; ++i) {
            const Tracker& t = *T[i];
            size_t* o = &rb_off[(size_t)5 * i];
            o[0] = rb; rb += 32;
            // a camera's list is its previous survivors plus at most one new point per grid cell
            for (int c = 0; c < 2; ++c)
                bnd[2 * i + c] = std::min((size_t)t.cap, (size_t)t.host_count[c] + (size_t)t.n_cells);
            for (int c = 0; c < 2; ++c) {
                o[1 + c] = rb; rb = up32(rb + bnd[2 * i + c] * sizeof(rsvio_feature));
            }
            for (int c = 0; c < 2; ++c) {
                o[3 + c] = rb; rb = up32(rb + (t.cams.on ? bnd[2 * i + c] * sizeof(float2) : 0));
            }
        }
        if (h_rb.n < rb) {
            h_rb.alloc(rb + rb / 2);
            d_rb.alloc(rb + rb / 2);
        }
        // the tables
        PyrSlot* ps = hp<PyrSlot>(off_pyr);
        rsvio_track_batch* lk = hp<rsvio_track_batch>(off_lk);
        const int4** mk = hp<const int4*>(off_mask);
        BatchSlot* bs = hp<BatchSlot>(off_slot);
        int32_t* st = hp<int32_t>(off_start);
        int nb = 0, k_host = 0;
        bool any_gate = false;
        st[0] = 0;
        for (int i = 0; i < n; ++i) {
            Tracker& t = *T[i];
            const int cur = t.cur, nxt = t.has_prev ? 1 - t.cur : t.cur;
            const uint8_t* src[2];
            if (f[i].on_device) {
                src[0] = f[i].left;
                src[1] = f[i].right;
            } else {
                const size_t stride = f[i].stride ? f[i].stride : w;
                for (int c = 0; c < 2; ++c) {
                    const size_t off = off_img + (size_t)(k_host++) * img_stride;
                    const uint8_t* im = c == 0 ? f[i].left : f[i].right;
                    if (stride == w)
                        std::memcpy(h_up.p + off, im, w * h);
                    else
                        for (size_t y = 0; y < h; ++y) std::memcpy(h_up.p + off + y * w, im + y * stride, w);
                    src[c] = d_up.p + off;
                }
            }
            ps[2 * i] = PyrSlot{src[0], t.pyr(nxt, 0), t.cell_pt.p, t.new_aff.p};
            ps[2 * i + 1] = PyrSlot{src[1], t.pyr(nxt, 1), nullptr, nullptr};
            auto add = [&](const uint8_t* p0, const uint8_t* p1, const float* ain, float* aout, uint8_t* valid, int cnt,
                           const int4* mask) {
                if (cnt <= 0) return;
                lk[nb] = rsvio_track_batch{p0, p1, ain, aout, valid, cnt};
                mk[nb] = mask;
                st[nb + 1] = st[nb] + cnt;
                ++nb;
            };
            if (t.has_prev)
                for (int c = 0; c < 2; ++c)
                    add(t.pyr(cur, c), t.pyr(nxt, c), t.maff(c), t.taff(c), t.valid.p + (size_t)c * t.cap,
                        t.host_count[c], nullptr);
            add(t.pyr(nxt, 0), t.pyr(nxt, 1), t.new_aff.p, t.new_aff1.p, t.new_valid.p, t.n_cells, t.cell_pt.p);
            BatchSlot& s = bs[i];
            s.bins = t.bins.p;
            s.n0 = t.host_count[0]; s.n1 = t.host_count[1]; s.tracked = t.has_prev ? 1 : 0; s.capacity = t.cap;
            s.at0 = t.taff(0); s.at1 = t.taff(1);
            s.tv0 = t.valid.p; s.tv1 = t.valid.p + t.cap;
            s.ids_tmp = t.ids_tmp.p;
            s.cell_pt = t.cell_pt.p;
            s.new_aff0 = t.new_aff.p; s.new_aff1 = t.new_aff1.p; s.new_valid = t.new_valid.p;
            s.map_aff0 = t.maff(0); s.map_aff1 = t.maff(1);
            s.ids0 = t.mid(0); s.ids1 = t.mid(1);
            s.counts = t.counts.p; s.last_id = t.last_id.p;
            s.out0 = t.outp(t.wslot, 0); s.out1 = t.outp(t.wslot, 1);
            s.overflow = t.overflow.p;
            s.und0 = t.undp(t.wslot, 0); s.und1 = t.undp(t.wslot, 1);
            const size_t* o = &rb_off[(size_t)5 * i];
            s.rb_head = reinterpret_cast<int*>(d_rb.p + o[0]);
            for (int c = 0; c < 2; ++c) {
                s.rb[c] = reinterpret_cast<rsvio_feature*>(d_rb.p + o[1 + c]);
                s.rbu[c] = reinterpret_cast<float2*>(d_rb.p + o[3 + c]);
                s.bnd[c] = (int)bnd[2 * i + c];
            }
            s.cams = t.cams;
            s.gate = t.gate_dev(t.wslot);
            any_gate = any_gate || t.gated();
        }
        const int total = st[nb];
        // ONE upload, three launches, ONE read-back, ONE wait
        RSVIO_HIP(hipMemcpyAsync(d_up.p, h_up.p, off_img + (size_t)k_host * img_stride, hipMemcpyHostToDevice, stream));
        if (device_ms) RSVIO_HIP(hipEventRecord(ev[0], stream));
        {
            PyrIO io{};
            io.table = dp<PyrSlot>(off_pyr);
            io.fast_cells = t0.n_cells;
            io.fg = t0.G;
            t0.plan.enqueue(io, 2 * n, stream);
        }
        {
            TrackLaunch L{};
            L.w = t0.P.width; L.h = t0.P.height; L.levels = t0.P.levels; L.max_iter = t0.P.max_iterations;
            L.thresh = t0.P.convergence_threshold;
            L.nb = nb;
            L.start[0] = total;  // table mode: the grid size
            L.table = dp<rsvio_track_batch>(off_lk);
            L.tstart = dp<int32_t>(off_start);
            L.tmask = dp<const int4*>(off_mask);
            enqueue_track(L, stream);
        }
        hipLaunchKernelGGL(any_gate ? append_pack_batch_gate_kernel : append_pack_batch_kernel, dim3(n), dim3(1024),
                           0, stream, t0.G, t0.n_cells, dp<BatchSlot>(off_slot));
        RSVIO_HIP(hipGetLastError());
        if (device_ms) RSVIO_HIP(hipEventRecord(ev[1], stream));
        RSVIO_HIP(hipMemcpyAsync(h_rb.p, d_rb.p, rb, hipMemcpyDeviceToHost, stream));
        RSVIO_HIP(hipStreamSynchronize(stream));
        if (device_ms) {
            float ms = 0.f;
            RSVIO_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
            *device_ms = ms;
        }
        // the handles' host state as enqueue_frame, submit and fetch leave it, with the slot's lists
        // and status
        for (int i = 0; i < n; ++i) {
            Tracker& t = *T[i];
            t.cur = t.has_prev ? 1 - t.cur : t.cur;
            t.has_prev = true;
            const size_t* o = &rb_off[(size_t)5 * i];
            const int* head = reinterpret_cast<const int*>(h_rb.p + o[0]);
            const int slot = t.wslot;
            t.wslot ^= 1;
            t.rslot = slot;
            t.pred_on[slot] = false;  // (an unpredicted frame: prediction_report gives zeros)
            t.pred_n[slot][0] = t.pred_n[slot][1] = 0;
            t.host_count[0] = head[0];
            t.host_count[1] = head[1];
            t.set_report(head + 4);
            const size_t ml = std::min((size_t)std::max(head[0], 0), bnd[2 * i]);
            const size_t mr = std::min((size_t)std::max(head[1], 0), bnd[2 * i + 1]);
            t.coll_n[0] = (int)ml;
            t.coll_n[1] = (int)mr;
            const bool skip_l = !f[i].out_l && !f[i].cap_l, skip_r = !f[i].out_r && !f[i].cap_r;
            const size_t nl = skip_l ? ml : std::min(ml, f[i].cap_l), nr = skip_r ? mr : std::min(mr, f[i].cap_r);
            if (nl && !skip_l) std::memcpy(f[i].out_l, h_rb.p + o[1], nl * sizeof(rsvio_feature));
            if (nr && !skip_r) std::memcpy(f[i].out_r, h_rb.p + o[2], nr * sizeof(rsvio_feature));
            if (t.cams.on) {
                std::memcpy(t.hund(slot, 0), h_rb.p + o[3], ml * sizeof(float2));
                std::memcpy(t.hund(slot, 1), h_rb.p + o[4], mr * sizeof(float2));
            }
            t.last_n[0] = t.cams.on ? nl : 0;
            t.last_n[1] = t.cams.on ? nr : 0;
            f[i].n_l = nl;
            f[i].n_r = nr;
            if (head[2]) {
                set_last_error("StereoPatchTracker: new points exceed max_features; the excess was dropped (slot " +
                               std::to_string(i) + ")");
                f[i].status = RSVIO_ERR_CAPACITY;
            } else if (nl < ml || nr < mr) {
                set_last_error("StereoPatchTracker: feature list exceeds the output capacity (truncated; slot " +
                               std::to_string(i) + ")");
                f[i].status = RSVIO_ERR_CAPACITY;
            } else {
                f[i].status = RSVIO_OK;
            }
        }
        return (int)RSVIO_OK;
    }
};

}  // namespace rsvio

struct rsvio_tracker_batch {
    rsvio::TrackerBatch b;
};

extern "C" {

int rsvio_tracker_batch_create(rsvio_tracker* const* handles, int32_t n, rsvio_tracker_batch** out) {
    if (!handles || !out || n < 1 || n > 1024) return RSVIO_ERR_INVALID_ARG;
    return guarded([&] {
        for (int i = 0; i < n; ++i) {
            const std::string at = "rsvio_tracker_batch_create: slot " + std::to_string(i) + ": ";
            if (!handles[i]) throw std::invalid_argument(at + "NULL handle");
            for (int j = 0; j < i; ++j)
                if (handles[j] == handles[i])
                    throw std::invalid_argument(at + "the handle of slot " + std::to_string(j) +
                                                " again (a handle may sit in one slot only)");
            if (!rsvio::same_params(handles[i]->t.P, handles[0]->t.P))
                throw std::invalid_argument(at + "parameters or device differ from slot 0's");
        }
        auto* h = new rsvio_tracker_batch();
        try {
            h->b.init(handles, n);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
        return (int)RSVIO_OK;
    });
}

int rsvio_tracker_batch_process_frames(rsvio_tracker_batch* b, rsvio_stereo_frame* frames, double* device_ms) {
    if (!b || !frames) return RSVIO_ERR_INVALID_ARG;
    return guarded([&] { return b->b.run(frames, device_ms); });
}

void rsvio_tracker_batch_destroy(rsvio_tracker_batch* b) { delete b; }

int rsvio_tracker_device_lists(rsvio_tracker* t, const rsvio_feature** d_l, size_t* n_l, const rsvio_feature** d_r,
                               size_t* n_r, const float** d_uv_l, const float** d_uv_r) {
    if (!t || !d_l || !n_l || !d_r || !n_r) return RSVIO_ERR_INVALID_ARG;
    const rsvio::TrackerView v = rsvio::tracker_view(t);
    *d_l = v.out[0];
    *d_r = v.out[1];
    *n_l = (size_t)v.n[0];
    *n_r = (size_t)v.n[1];
    if (d_uv_l) *d_uv_l = reinterpret_cast<const float*>(v.undist[0]);
    if (d_uv_r) *d_uv_r = reinterpret_cast<const float*>(v.undist[1]);
    return RSVIO_OK;
}

}  // extern "C"
