// Framing of centred STFT frames (librosa.stft's reflect padding by N / 2), device side only: the one reflection and the one span clamp
// every framing kernel uses, and the LDS-staged core of ssv_span_frames (dvector.hip), ssv_tisv_frames_table (sv_frontend.hip) and
// ssv_preemph_frames_ragged (corpus_features.hip).  ssv_tisv_frames and ssv_frame_signal are still direct gathers.
#pragma once

// index into a row of len samples of position j of the row reflect-padded without repeating its end samples; one reflection:
// -len < j < 2 * len - 1
__device__ __forceinline__ int ssv_reflect(int j, int len) { return j < 0 ? -j : (j >= len ? 2 * (len - 1) - j : j); }

// a DEVICE (start, end) pair is not trusted: 0 <= start <= end <= n_max afterwards
__device__ __forceinline__ void ssv_clamp_span(int& start, int& end, int n_max) {
  start = start < 0 ? 0 : (start > n_max ? n_max : start);
  end = end < start ? start : (end > n_max ? n_max : end);
}

// LDS image of a tile's staged sample range: sample s at s + (s >> sh), hop = 2^sh * q with q odd (sh = 31, no skew, for an odd hop).
// Lane t of a wave reads sample t * hop + i, which lands at t * (hop + q) + i + (i >> sh): the lane stride hop + q is odd, so the 32
// lanes of a ds_read_b32 group meet 32 different banks (hop = 256: stride 257; hop = 160, sh = 5: stride 165 -- unskewed, all 32 lanes
// would meet in ONE bank).  A fixed sh = 5 is conflict-free for every hop = 32 q with q odd; other hops are merely correct.  The image of
// count samples takes count + (count >> sh) + 1 floats at the most.
__device__ __forceinline__ int ssv_skew(int s, int sh) { return s + (s >> sh); }

// The tile's samples, staged ONCE: sm[skew(s)] = reflect_pad(p, N / 2)[lo + s] for s < count, p = seg[0 .. len) (PREEMPH: its
// pre-emphasis, p[0] = seg[0], p[j] = seg[j] - a * seg[j - 1] as one fused multiply-add, a single fp32 rounding that never reaches
// memory; the sample before seg[0] is not read).  Coalesced; the reflection is applied on the way in (frames overlap by 1 - hop / N).
// The workgroup has THREADS threads; the caller owns sm and the barrier after this, and has checked that len > N / 2 and that the
// tile's last frame starts at or before len, so that one reflection gives 0 <= j < len.
template <bool PREEMPH, int THREADS>
__device__ __forceinline__ void frame_stage_load(float* sm, const float* __restrict__ seg, int len, int lo, int count, int sh, float a) {
  for (int s = threadIdx.x; s < count; s += THREADS) {
    int j = ssv_reflect(lo + s, len);
    if constexpr (PREEMPH) {
      j = j < 0 ? 0 : (j >= len ? len - 1 : j);             // (kept in bounds whatever the caller's sizes)
      const float x = seg[j];
      sm[ssv_skew(s, sh)] = j > 0 ? fmaf(-a, seg[j - 1], x) : x;
    } else {                                                // no clamp: the caller has checked the conditions above on its own table row,
      sm[ssv_skew(s, sh)] = seg[j];                         // and with one hipcc unrolls this loop by 4 instead of 8 (loads in flight)
    }
  }
}

// One frame of the staged tile, written out: sample rows first_row, first_row + row_step, ... < N of the frame whose first staged sample
// is s0 (= its index in the tile times hop) go to dst[row * stride].  The threads of a wave hold consecutive frames, so each row of the
// tile leaves as one run.
__device__ __forceinline__ void frame_stage_store(const float* sm, float* __restrict__ dst, int stride, int s0, int first_row, int row_step,
                                                  int N, int sh) {
#pragma unroll 4
  for (int i = first_row; i < N; i += row_step) dst[(long)i * stride] = sm[ssv_skew(s0 + i, sh)];
}
