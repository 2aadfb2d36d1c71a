// lk_track.hpp -- K2 launch descriptor (see lk_track.hip).
#pragma once
#include "common.hpp"

namespace rsvio {

constexpr int kMaxTrackBatches = 4;

// Up to 4 independent track_points batches (e.g. cam0 and cam1 temporal tracking) per launch;
// one 64-lane workgroup per feature.
struct TrackLaunch {
    uint32_t w, h;
    int levels;
    int max_iter;
    float thresh;
    int nb;
    int start[kMaxTrackBatches + 1];           // prefix of batch sizes (launch capacity)
    const uint8_t* pyr0[kMaxTrackBatches];
    const uint8_t* pyr1[kMaxTrackBatches];
    const float* ain[kMaxTrackBatches];        // n x 6 {m11, m12, m21, m22, m13, m23}
    float* aout[kMaxTrackBatches];
    uint8_t* valid[kMaxTrackBatches];
    const int* dcount[kMaxTrackBatches];       // optional device-side count (early exit)
    const int4* mask[kMaxTrackBatches];        // optional: job i runs only when mask[i].w != 0 (else valid = 0)
    // batched serving mode (rsvio_track_points_table_d): when set, batch descriptors and the
    // prefix of their sizes come from device memory and nb may exceed kMaxTrackBatches
    const rsvio_track_batch* table;
    const int32_t* tstart;
    // table mode's job masks (the batched tracker's stereo cell jobs): a device array of nb mask
    // pointers, entry b as mask[] above for table batch b (null entry: no mask); null: none
    const int4* const* tmask;
    int njobs;  // set by enqueue_track: jobs in this launch
};

void enqueue_track(const TrackLaunch& L, hipStream_t s);

// Seeded launch (lk_track_seeded_kernel): the same jobs, each feature's search started at a seed
// instead of its own position.  A launch argument of its own beside TrackLaunch, so the unseeded
// kernels' argument block is what it was.
struct TrackSeeds {
    const float* seed[kMaxTrackBatches];  // per batch: n x 2 f32 start positions; null: its own position
    const float* const* tseed;            // table mode: a device array of nb seed pointers (null entry: as above)
};

void enqueue_track_seeded(const TrackLaunch& L, const TrackSeeds& S, hipStream_t s);

}  // namespace rsvio
