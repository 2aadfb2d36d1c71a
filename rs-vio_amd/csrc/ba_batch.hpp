// ba_batch.hpp -- HP-B batched mode, host side: B window handles (their problems uploaded by
// rsvio_ba_set_problem) run, triangulated, checked and given covariances by one launch chain per
// call on the batch's stream, over tables whose rows the handles fill themselves (fill_desc,
// lm_plan, cov_plan).  The host reads the B LM states once per chunk.  A window's own stream is
// never synchronised from the host: the batch stream waits for it on the device (after_window).
//
// A fragment of ba.hip, included by ba.hip inside namespace rsvio after BundleAdjuster (not a
// header of its own).
#pragma once

struct BundleBatch {
    std::vector<BundleAdjuster*> win;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf<WinDesc> d_desc;
    HostBuf<WinDesc> h_desc;
    HostBuf<LmState> h_states;
    DevBuf<int> d_dmap;
    HostBuf<int> h_dmap;
    std::vector<hipEvent_t> ev_win;  // per window: its stream's pending work (an upload) before the batch
    int last_iterations = 3;
    // the batched keyframe step (triangulate, check, covariance): the landmark kernels' table has
    // its own pinned image and an event for its upload, because an enqueue-only triangulate
    // returns before the copy has read it; the covariance's status words and costs sit in one
    // array of the batch (one read-back for all windows), its other scratch is each handle's
    DevBuf<LmDesc> d_lmdesc;
    HostBuf<LmDesc> h_lmdesc;
    hipEvent_t ev_lmcopy = nullptr, ev_after = nullptr;
    bool lmcopy_pending = false;
    DevBuf<CovDesc> d_covdesc;
    HostBuf<CovDesc> h_covdesc;
    DevBuf<int> d_cst;
    HostBuf<int> h_cst;
    DevBuf<double> d_cost;
    HostBuf<double> h_cost;

    void init(BundleAdjuster* const* w, int n) {
        if (n < 1) throw std::invalid_argument("a batch needs at least one window");
        for (int i = 0; i < n; ++i) {
            if (!w[i]) throw std::invalid_argument("null window handle");
            if (i && w[i]->P.device != w[0]->P.device) throw std::invalid_argument("windows on different devices");
            if (w[i]->sharded()) throw std::invalid_argument("a sharded window cannot join a batch");
            for (int j = 0; j < i; ++j)  // two grid rows on one set of state buffers would race
                if (w[j] == w[i]) throw std::invalid_argument("a window handle appears twice in the batch");
            win.push_back(w[i]);
        }
        device = w[0]->P.device;
        RSVIO_HIP(hipSetDevice(device));
        RSVIO_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        RSVIO_HIP(hipEventCreate(&ev0));
        RSVIO_HIP(hipEventCreate(&ev1));
        ev_win.assign(n, nullptr);
        for (int i = 0; i < n; ++i) RSVIO_HIP(hipEventCreateWithFlags(&ev_win[i], hipEventDisableTiming));
        d_desc.alloc(n);
        h_desc.alloc(n);
        h_states.alloc(n, hipHostMallocCoherent);
        RSVIO_HIP(hipEventCreateWithFlags(&ev_lmcopy, hipEventDisableTiming));
        RSVIO_HIP(hipEventCreateWithFlags(&ev_after, hipEventDisableTiming));
        d_lmdesc.alloc(n);
        h_lmdesc.alloc(n);
        d_covdesc.alloc(n);
        h_covdesc.alloc(n);
        d_cst.alloc(2 * (size_t)n);
        h_cst.alloc(2 * (size_t)n);
        d_cost.alloc(n);
        h_cost.alloc(n);
    }
    ~BundleBatch() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (ev_lmcopy) (void)hipEventDestroy(ev_lmcopy);
        if (ev_after) (void)hipEventDestroy(ev_after);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        for (hipEvent_t e : ev_win)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // the table's launches; K4 / K6 as wide as the widest window, rounded up to kGrp (wave w on XCD w % 8)
    DescChain chain(int max_wave, int max_chunk) const {
        return DescChain{stream, d_desc.p, (int)win.size(), (max_wave + kGrp - 1) / kGrp * kGrp, max_chunk};
    }

    void launch_k5(int nf, int wi) {
        const int B = (int)win.size();
        const bool k5 = dispatch_panel_nf(nf, [&](auto c) {
            constexpr int NF = decltype(c)::value;
            hipLaunchKernelGGL(bab_camera_solve<NF>, dim3(B), dim3(kK5Threads), 0, stream, d_desc.p, wi);
        }) || dispatch_block_nf(nf, [&](auto c) {
            constexpr int NF = decltype(c)::value;
            hipLaunchKernelGGL(bab_camera_solve_blk<NF>, dim3(B), dim3(64 * kBkWaves), 0, stream, d_desc.p, wi);
        });
        if (!k5) throw std::logic_error("batched mode: no camera-solve template for this window size");
        RSVIO_HIP(hipGetLastError());
    }

    // on: one byte per window (null = every window).  A window that is off is a skipped row of the
    // descriptor table: it is not read, written or required to hold a problem, and res[i] is left.
    void run(const rsvio_lm_cfg& cfg, rsvio_ba_result* res, const uint8_t* on = nullptr) {
        const int B = (int)win.size();
        int nf = 1, max_wave = 1, max_chunk = 1, active = 0;
        std::vector<int> skip(B, 0);
        size_t ne_total = 0;
        for (int i = 0; i < B; ++i) {
            if (on && !on[i]) continue;
            const BundleAdjuster& w = *win[i];
            const std::string slot = on ? " (window " + std::to_string(i) + ")" : std::string();
            if (w.pend.active)
                throw CallOrderError("rsvio_ba_batch_run: a solve is in flight (call rsvio_ba_wait first)" + slot);
            if (!w.has_problem) throw std::invalid_argument("batch window without a problem" + slot);
        }
        for (int i = 0; i < B; ++i) {
            if (on && !on[i]) {
                skip[i] = 2;
                continue;
            }
            BundleAdjuster& w = *win[i];
            w.state_export = false;  // the batch's decisions leave the state in device memory
            const Geometry& G = w.G;
            // as the single-window start(); a window without a wave has nothing to launch
            skip[i] = (w.underconstrained() || G.n_wave == 0) ? 1 : 0;
            if (skip[i]) continue;
            ++active;
            nf = std::max(nf, G.n_free);
            max_wave = std::max(max_wave, G.n_wave);
            max_chunk = std::max(max_chunk, G.n_chunk);
            ne_total += (size_t)36 * G.n_pb + 12 * G.n_free;
        }
        // past 10 free keyframes every window runs the 6x6-block solver's padded template
        if (nf > 10) nf = bk_template_nf(nf);
        // descriptors and the camera-solve maps for the batch's template (b row at 6 nf)
        if (h_dmap.n < std::max<size_t>(ne_total, 1)) {
            h_dmap.alloc(ne_total + 1);
            d_dmap.alloc(ne_total + 1);
        }
        size_t off = 0;
        for (int i = 0; i < B; ++i) {
            BundleAdjuster& w = *win[i];
            WinDesc& d = h_desc.p[i];
            if (skip[i] == 2) {  // off: no field of the handle is read
                d = WinDesc{};
                d.skip = 1;
                continue;
            }
            w.fill_desc(d, cfg.huber_delta, cfg.linear_solver == RSVIO_SOLVER_CHOLESKY ? 1 : 0);
            d.skip = skip[i];
            if (skip[i]) {
                res[i] = rsvio_ba_result{};
                res[i].status = RSVIO_LM_SKIPPED;
                continue;
            }
            const size_t ne = (size_t)36 * w.G.n_pb + 12 * w.G.n_free;
            mf_dense_map(w.G.n_free, w.G.n_pb, w.hs_pb_fa.data(), w.hs_pb_fb.data(), h_dmap.p + off, 6 * nf,
                         nf > 10 ? kBkLd : kMfLd);
            d.Pr.dmap = d_dmap.p + off;
            off += ne;
        }
        if (!active) return;
        // the batch's kernels read what each window's stream may still be writing (set_problem's
        // upload and ba_build_layout are asynchronous)
        for (int i = 0; i < B; ++i)
            if (skip[i] != 2) after_window(i);
        RSVIO_HIP(hipMemcpyAsync(d_dmap.p, h_dmap.p, sizeof(int) * std::max<size_t>(off, 1), hipMemcpyHostToDevice, stream));
        RSVIO_HIP(hipMemcpyAsync(d_desc.p, h_desc.p, sizeof(WinDesc) * B, hipMemcpyHostToDevice, stream));
        RSVIO_HIP(hipEventRecord(ev0, stream));
        const DescChain ch = chain(max_wave, max_chunk);
        ch.linearize(cfg.lambda_init);
        RSVIO_HIP(hipGetLastError());
        const LmArgs la = BundleAdjuster::lm_args(cfg);
        const int max_it = std::max(cfg.max_iterations, 1);
        int enq = 0;
        int k = BundleAdjuster::first_chunk(last_iterations, max_it);
        int max_iter_seen = 0;
        while (true) {
            for (int i = 0; i < k; ++i, ++enq) {
                const int wi = enq & 1;
                ch.schur(wi, la);
                RSVIO_HIP(hipGetLastError());
                launch_k5(nf, wi);
                ch.backsub(wi);
                RSVIO_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(bab_lm_decide, dim3(B), dim3(64), 0, stream, d_desc.p, 2 + (enq & 1), la, h_states.p);
            RSVIO_HIP(hipGetLastError());
            RSVIO_HIP(hipEventRecord(ev1, stream));
            RSVIO_HIP(hipStreamSynchronize(stream));
            bool all_done = true;
            for (int i = 0; i < B; ++i)
                if (!skip[i]) {
                    all_done = all_done && h_states.p[i].done;
                    max_iter_seen = std::max(max_iter_seen, h_states.p[i].iter);
                }
            if (all_done || enq >= max_it) break;
            k = std::min(2, max_it - enq);
        }
        float ms = 0.0f;
        RSVIO_HIP(hipEventElapsedTime(&ms, ev0, ev1));
        last_iterations = std::max(max_iter_seen, 1);
        for (int i = 0; i < B; ++i) {
            if (skip[i]) continue;
            BundleAdjuster& w = *win[i];
            const LmState& st = h_states.p[i];
            *w.h_state.p = st;
            w.state_fresh = false;
            w.at_initial = false;
            // the window's stream ran nothing after the event the batch waited on, and the batch
            // stream is synchronised: both are idle
            w.settled = true;
            w.destroy_retired();
            w.last_iterations = st.iter;
            BundleAdjuster::fill_result(res[i], st, ms);
        }
    }

    // the batch stream waits, on the device, for what window i's own stream still has enqueued
    void after_window(int i) {
        BundleAdjuster& w = *win[i];
        if (w.settled) return;
        RSVIO_HIP(hipEventRecord(ev_win[i], w.stream));
        RSVIO_HIP(hipStreamWaitEvent(stream, ev_win[i], 0));
    }
    // after a host wait on the batch stream: window i's stream ran nothing since after_window
    void idle_window(int i) {
        BundleAdjuster& w = *win[i];
        w.settled = true;
        w.sel_pending = false;
        w.destroy_retired();
    }

    // rsvio_ba_batch_triangulate (tri) / _check_landmarks: BundleAdjuster::landmarks per slot, by
    // one bab_landmarks launch.  The gates were validated by the caller (gate[i]: slot i's).
    void landmarks(bool tri, const uint8_t* on, const std::vector<const rsvio_landmark_gate*>& gate,
                   rsvio_ba_landmark_slot* slots, double* device_ms) {
        const char* what = tri ? "rsvio_ba_batch_triangulate" : "rsvio_ba_batch_check_landmarks";
        const int B = (int)win.size();
        int n_act = 0;
        bool want = !tri;
        for (int i = 0; i < B; ++i) {
            if (on && !on[i]) continue;
            win[i]->lm_check(what, slots[i].n_lm, i);
            ++n_act;
            want = want || (tri && slots[i].p_W_out) || slots[i].info_out;
        }
        if (device_ms) *device_ms = 0.0;
        if (!n_act) return;
        if (lmcopy_pending) RSVIO_HIP(hipEventSynchronize(ev_lmcopy));  // the last upload has read the image
        lmcopy_pending = false;
        int max_blocks = 0;
        for (int i = 0; i < B; ++i) {
            LmDesc& d = h_lmdesc.p[i];
            d = LmDesc{};
            d.skip = 1;
            if (on && !on[i]) continue;
            BundleAdjuster& w = *win[i];
            slots[i].n_ok = want ? 0 : -1;
            slots[i].status = RSVIO_OK;
            if (!w.G.n_lm) continue;
            d = w.lm_plan(tri, slots[i].lm_mask, *gate[i]);
            max_blocks = std::max(max_blocks, w.G.n_wave + (w.G.n_lm + 63) / 64);
        }
        if (!max_blocks) return;
        for (int i = 0; i < B; ++i)
            if (!h_lmdesc.p[i].skip) after_window(i);
        RSVIO_HIP(hipMemcpyAsync(d_lmdesc.p, h_lmdesc.p, sizeof(LmDesc) * B, hipMemcpyHostToDevice, stream));
        RSVIO_HIP(hipEventRecord(ev_lmcopy, stream));
        lmcopy_pending = true;
        RSVIO_HIP(hipEventRecord(ev0, stream));
        with_tri(tri, [&](auto t) {
            hipLaunchKernelGGL(bab_landmarks<decltype(t)::value>, dim3(max_blocks, B), dim3(64), 0, stream, d_lmdesc.p);
        });
        RSVIO_HIP(hipGetLastError());
        RSVIO_HIP(hipEventRecord(ev1, stream));
        for (int i = 0; i < B; ++i) {
            if (h_lmdesc.p[i].skip) continue;
            BundleAdjuster& w = *win[i];
            w.settled = false;
            if (h_lmdesc.p[i].sel) {
                RSVIO_HIP(hipEventRecord(w.ev_sel, stream));
                w.sel_pending = true;
            }
        }
        if (!want) {
            // enqueue only: whatever a window's own stream runs next comes after the batch's kernel
            RSVIO_HIP(hipEventRecord(ev_after, stream));
            for (int i = 0; i < B; ++i)
                if (!h_lmdesc.p[i].skip) RSVIO_HIP(hipStreamWaitEvent(win[i]->stream, ev_after, 0));
            return;
        }
        for (int i = 0; i < B; ++i) {
            if (h_lmdesc.p[i].skip) continue;
            BundleAdjuster& w = *win[i];
            const size_t n_lm = (size_t)w.G.n_lm;
            if (tri && slots[i].p_W_out)
                RSVIO_HIP(hipMemcpyAsync(slots[i].p_W_out, h_lmdesc.p[i].pw_out, sizeof(double) * 3 * n_lm,
                                         hipMemcpyDeviceToHost, stream));
            RSVIO_HIP(hipMemcpyAsync(w.h_lm_info.p, w.d_lm_info.p, sizeof(rsvio_landmark_info) * n_lm,
                                     hipMemcpyDeviceToHost, stream));
        }
        RSVIO_HIP(hipStreamSynchronize(stream));
        lmcopy_pending = false;
        float ms = 0.0f;
        RSVIO_HIP(hipEventElapsedTime(&ms, ev0, ev1));
        if (device_ms) *device_ms = ms;
        for (int i = 0; i < B; ++i) {
            if (h_lmdesc.p[i].skip) continue;
            idle_window(i);
            win[i]->lm_deliver(slots[i].info_out, &slots[i].n_ok);
        }
    }

    // rsvio_ba_batch_covariance: BundleAdjuster::covariance per slot by one launch chain -- K4 and
    // K4c on a table of each window's covariance views, the camera covariance once per distinct
    // template among the windows, the landmark covariance -- and two host waits: the statuses and
    // costs, then the outputs of the windows that report OK.
    void covariance(const uint8_t* on, double huber_delta, rsvio_ba_cov_slot* slots, double* device_ms) {
        const std::string what = "rsvio_ba_batch_covariance";
        const int B = (int)win.size();
        if (!(huber_delta > 0.0)) throw std::invalid_argument(what + ": huber_delta must be positive");
        int n_act = 0;
        for (int i = 0; i < B; ++i) {
            if (on && !on[i]) continue;
            const BundleAdjuster& w = *win[i];
            const std::string slot = what + " (slot " + std::to_string(i) + ")";
            if (w.sharded()) throw std::invalid_argument(slot + ": not available on a landmark-sharded handle");
            w.cov_check(slot, huber_delta, slots[i].lm_idx, slots[i].n_sel, slots[i].cov_lm, slots[i].lm_flags);
            ++n_act;
        }
        if (device_ms) *device_ms = 0.0;
        if (!n_act) return;
        int max_wave = 1, max_chunk = 1, max_blocks = 1;
        std::vector<int> tmpl;  // the distinct camera templates, in order of first appearance
        for (int i = 0; i < B; ++i) {
            WinDesc& d = h_desc.p[i];
            CovDesc& c = h_covdesc.p[i];
            d = WinDesc{};
            c = CovDesc{};
            d.skip = 1;
            if (on && !on[i]) continue;
            BundleAdjuster& w = *win[i];
            const BundleAdjuster::CovPlan p = w.cov_plan(huber_delta, slots[i].lm_idx, slots[i].n_sel);
            d.skip = 0;
            d.G = p.Gc;
            d.Pr = p.pr;
            d.W[0] = d.W[1] = p.wk;
            d.W[2] = d.W[3] = p.wl;
            c.O = p.O;
            c.O.cst = d_cst.p + 2 * i;
            c.O.cost = d_cost.p + i;
            c.obs_mask = w.obs_mask_dev();
            c.sel = p.d_sel;
            const int nf = w.G.n_free;
            c.nf = nf <= 10 ? nf : bk_template_nf(nf);
            if (c.nf > 0 && std::find(tmpl.begin(), tmpl.end(), c.nf) == tmpl.end()) tmpl.push_back(c.nf);
            max_wave = std::max(max_wave, w.G.n_wave);
            max_chunk = std::max(max_chunk, w.G.n_chunk);
            max_blocks = std::max(max_blocks, w.G.n_wave + (w.G.n_lm + 63) / 64);
        }
        for (int i = 0; i < B; ++i)
            if (!h_desc.p[i].skip) after_window(i);
        RSVIO_HIP(hipMemcpyAsync(d_desc.p, h_desc.p, sizeof(WinDesc) * B, hipMemcpyHostToDevice, stream));
        RSVIO_HIP(hipMemcpyAsync(d_covdesc.p, h_covdesc.p, sizeof(CovDesc) * B, hipMemcpyHostToDevice, stream));
        RSVIO_HIP(hipMemsetAsync(d_cst.p, 0, sizeof(int) * 2 * B, stream));
        RSVIO_HIP(hipEventRecord(ev0, stream));
        const DescChain ch = chain(max_wave, max_chunk);
        ch.linearize(0.0);
        ch.schur(0, LmArgs{1, 0.0, 0.0});
        for (int nf : tmpl) {
            auto launch = [&](auto c) {
                constexpr int NF = decltype(c)::value;
                hipLaunchKernelGGL(bab_camera_covariance<NF>, dim3(B), dim3(NF <= 10 ? kK5Threads : 64 * kBkWaves), 0,
                                   stream, d_desc.p, d_covdesc.p);
            };
            if (!(dispatch_panel_nf(nf, launch) || dispatch_block_nf(nf, launch)))
                throw std::logic_error("batched covariance: no camera template for this window size");
        }
        hipLaunchKernelGGL(bab_landmark_covariance, dim3(max_blocks, B), dim3(64), 0, stream, d_desc.p, d_covdesc.p);
        RSVIO_HIP(hipGetLastError());
        RSVIO_HIP(hipEventRecord(ev1, stream));
        for (int i = 0; i < B; ++i) {
            if (h_desc.p[i].skip) continue;
            win[i]->settled = false;
            RSVIO_HIP(hipMemsetAsync(win[i]->d_singular.p, 0, sizeof(int), stream));  // K4c may have set it
        }
        RSVIO_HIP(hipMemcpyAsync(h_cst.p, d_cst.p, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, stream));
        RSVIO_HIP(hipMemcpyAsync(h_cost.p, d_cost.p, sizeof(double) * B, hipMemcpyDeviceToHost, stream));
        RSVIO_HIP(hipStreamSynchronize(stream));
        float ms = 0.0f;
        RSVIO_HIP(hipEventElapsedTime(&ms, ev0, ev1));
        if (device_ms) *device_ms = ms;
        bool any_ok = false;
        for (int i = 0; i < B; ++i) {
            if (h_desc.p[i].skip) continue;
            BundleAdjuster& w = *win[i];
            rsvio_ba_cov_slot& sl = slots[i];
            BundleAdjuster::cov_fill_info(&sl.info, w.G.n_free, h_cst.p + 2 * i, h_cost.p[i], ms);
            if (sl.info.status != RSVIO_COV_OK) continue;
            w.cov_fetch(h_covdesc.p[i].O, sl.cov_cc || sl.cov_pose, sl.n_sel, stream);
            any_ok = true;
        }
        if (any_ok) RSVIO_HIP(hipStreamSynchronize(stream));
        for (int i = 0; i < B; ++i) {
            if (h_desc.p[i].skip) continue;
            const rsvio_ba_cov_slot& sl = slots[i];
            if (sl.info.status == RSVIO_COV_OK)
                win[i]->cov_deliver(sl.cov_cc, sl.cov_pose, sl.lm_idx, sl.n_sel, sl.cov_lm, sl.lm_flags);
            idle_window(i);
        }
    }
};
