// C-ABI entries of the full-covariance UBM (include/ssv_hip.h, "I-vector groundwork: full-covariance UBM"): the argument checks, the
// run counts and the workspace layouts, all before any launch and without a device; the kernels are in fgmm.hip, the limits, the two tile
// sizes and the launchers' declarations in ivec_chain.h.
#include "ssv_host.h"
#include "ivec_chain.h"

#define FGMM_POST_RUNS 16           // most runs a list is split into by the likelihood kernel ...
#define FGMM_STATS_RUNS 8           // ... and by the statistics, whose slab grows with them

static int fgmm_cd_ok(const char* what, int C, int D) {
  SSV_CHECK(C >= 1 && D >= 1, SSV_BAD_SHAPE, "%s: need C >= 1 and D >= 1; got C=%d D=%d", what, C, D);
  SSV_CHECK(C <= IVEC_MAX_C && D <= IVEC_MAX_D, SSV_UNSUPPORTED, "%s: C=%d (at most %d) or D=%d (at most %d) beyond the kernels", what, C, IVEC_MAX_C, D, IVEC_MAX_D);
  return 0;
}

static int fgmm_sel_ok(const char* what, long F, int nsel, int C, int D) {
  SSV_CHECK(F >= 1 && nsel >= 1, SSV_BAD_SHAPE, "%s: need F >= 1 and nsel >= 1; got F=%ld nsel=%d", what, F, nsel);
  SSV_TRY(fgmm_cd_ok(what, C, D));
  SSV_CHECK(nsel <= IVEC_MAX_NSEL, SSV_UNSUPPORTED, "%s: nsel=%d beyond %d", what, nsel, IVEC_MAX_NSEL);
  SSV_CHECK(F <= 0x7fffffffL / nsel, SSV_UNSUPPORTED, "%s: %ld frames x %d selected exceed the int32 slots", what, F, nsel);
  return 0;
}

// runs a Gaussian's list is split into: from the shapes alone, about one run per mean list length of a tile, at most cap
static int fgmm_runs(long F, int nsel, int C, int cap) {
  const long r = F * nsel / ((long)C * FGMM_TILE);
  return (int)(r < 1 ? 1 : r > cap ? cap : r);
}

extern "C" int ssv_fgmm_pair_tile(void) { return FGMM_TILE; }

extern "C" int ssv_fgmm_stats_runs(long F, int nsel, int C) {
  if (F < 1 || nsel < 1 || nsel > IVEC_MAX_NSEL || C < 1 || C > IVEC_MAX_C || F > 0x7fffffffL / nsel) return 0;
  return fgmm_runs(F, nsel, C, FGMM_STATS_RUNS);
}

extern "C" long ssv_fgmm_group_workspace(long F, int nsel, int C) {
  if (F < 1 || nsel < 1 || nsel > IVEC_MAX_NSEL || C < 1 || C > IVEC_MAX_C || F > 0x7fffffffL / nsel) return 0;
  return (long)align256((size_t)((F * nsel + FGMM_SL - 1) / FGMM_SL) * C * sizeof(int));
}

extern "C" long ssv_fgmm_post_workspace(long F, int nsel) {
  if (F < 1 || nsel < 1 || nsel > IVEC_MAX_NSEL || F > 0x7fffffffL / nsel) return 0;
  return (long)align256((size_t)F * nsel * sizeof(float));
}

extern "C" long ssv_fgmm_stats_workspace(long F, int nsel, int C, int D) {
  const int runs = ssv_fgmm_stats_runs(F, nsel, C);
  if (!runs || D < 1 || D > IVEC_MAX_D) return 0;
  return (long)align256((size_t)runs * C * (1 + D + (size_t)D * (D + 1) / 2) * sizeof(float));
}

extern "C" int ssv_fgmm_planes(const double* w, const double* mu, const double* cov, float* Wt, float* muf, float* g, double* icov, int C, int D,
                               ssv_stream_t stream) {
  SSV_CHECK(w && mu && cov && Wt && muf && g && icov, SSV_BAD_SHAPE, "fgmm_planes: null pointer (w, mu, cov, Wt, muf, g and icov are required)");
  SSV_TRY(fgmm_cd_ok("fgmm_planes", C, D));
  return fgmm_launch_planes(w, mu, cov, Wt, muf, g, icov, C, D, (hipStream_t)stream);
}

extern "C" int ssv_fgmm_group_selection(const int* idx, int* start, int* pairs, long F, int nsel, int C, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(idx && start && pairs && ws, SSV_BAD_SHAPE, "fgmm_group_selection: null pointer (idx, start, pairs and ws are required)");
  SSV_TRY(fgmm_sel_ok("fgmm_group_selection", F, nsel, C, 1));
  SSV_CHECK(ws_bytes >= (size_t)ssv_fgmm_group_workspace(F, nsel, C), SSV_BAD_SHAPE, "fgmm_group_selection: workspace of %zu bytes, %ld needed", ws_bytes,
            ssv_fgmm_group_workspace(F, nsel, C));
  return fgmm_launch_group(idx, start, pairs, (int*)ws, F * nsel, C, (hipStream_t)stream);
}

extern "C" int ssv_fgmm_select_post(const float* X, const float* Wt, const float* muf, const float* g, const int* idx, const int* start, const int* pairs,
                                    float* post, float* loglik, long F, int D, int C, int nsel, float min_post, void* ws, size_t ws_bytes,
                                    ssv_stream_t stream) {
  SSV_CHECK(X && Wt && muf && g && idx && start && pairs && post && loglik && ws, SSV_BAD_SHAPE,
            "fgmm_select_post: null pointer (X, Wt, muf, g, idx, start, pairs, post, loglik and ws are required)");
  SSV_TRY(fgmm_sel_ok("fgmm_select_post", F, nsel, C, D));
  SSV_CHECK(min_post >= 0.f && min_post < 1.f, SSV_BAD_SHAPE, "fgmm_select_post: min_post=%g must lie in [0, 1)", (double)min_post);
  SSV_CHECK(ws_bytes >= (size_t)ssv_fgmm_post_workspace(F, nsel), SSV_BAD_SHAPE, "fgmm_select_post: workspace of %zu bytes, %ld needed", ws_bytes,
            ssv_fgmm_post_workspace(F, nsel));
  return fgmm_launch_post(X, Wt, muf, g, idx, start, pairs, post, loglik, (float*)ws, F, D, C, nsel, fgmm_runs(F, nsel, C, FGMM_POST_RUNS), min_post,
                          (hipStream_t)stream);
}

extern "C" int ssv_fgmm_stats(const float* X, const float* muf, const float* post, const int* start, const int* pairs, double* out, long F, int D, int C,
                              int nsel, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(X && muf && post && start && pairs && out && ws, SSV_BAD_SHAPE, "fgmm_stats: null pointer (X, muf, post, start, pairs, out and ws are required)");
  SSV_TRY(fgmm_sel_ok("fgmm_stats", F, nsel, C, D));
  SSV_CHECK(ws_bytes >= (size_t)ssv_fgmm_stats_workspace(F, nsel, C, D), SSV_BAD_SHAPE, "fgmm_stats: workspace of %zu bytes, %ld needed", ws_bytes,
            ssv_fgmm_stats_workspace(F, nsel, C, D));
  const int runs = fgmm_runs(F, nsel, C, FGMM_STATS_RUNS);
  SSV_TRY(fgmm_launch_stats(X, muf, post, start, pairs, (float*)ws, F, D, C, nsel, runs, (hipStream_t)stream));
  return ivec_launch_reduce((const float*)ws, out, runs, (long)C * (1 + D + (long)D * (D + 1) / 2), (hipStream_t)stream);
}

extern "C" int ssv_fgmm_update(const double* stats, double* w, double* mu, double* cov, float* Wt, float* muf, float* g, double* icov, int* kept, int C,
                               int D, double var_floor, double min_count, double min_weight, ssv_stream_t stream) {
  SSV_CHECK(stats && w && mu && cov && Wt && muf && g && icov && kept, SSV_BAD_SHAPE,
            "fgmm_update: null pointer (stats, w, mu, cov, Wt, muf, g, icov and kept are required)");
  SSV_TRY(fgmm_cd_ok("fgmm_update", C, D));
  SSV_CHECK(var_floor > 0.0 && min_weight > 0.0 && min_weight < 1.0 && min_count >= 0.0, SSV_BAD_SHAPE,
            "fgmm_update: need var_floor > 0, min_count >= 0 and 0 < min_weight < 1; got %g, %g, %g", var_floor, min_count, min_weight);
  return fgmm_launch_update(stats, w, mu, cov, Wt, muf, g, icov, kept, C, D, var_floor, min_count, min_weight, (hipStream_t)stream);
}

extern "C" int ssv_ivec_tv_planes_full(const double* T, const double* icov, float* G, float* Pk, int C, int D, int R, ssv_stream_t stream) {
  SSV_CHECK(T && icov && G && Pk, SSV_BAD_SHAPE, "ivec_tv_planes_full: null pointer (T, icov, G and Pk are required)");
  SSV_CHECK(R >= 1, SSV_BAD_SHAPE, "ivec_tv_planes_full: need R >= 1; got R=%d", R);
  SSV_TRY(fgmm_cd_ok("ivec_tv_planes_full", C, D));
  SSV_CHECK(R <= IVEC_MAX_R, SSV_UNSUPPORTED, "ivec_tv_planes_full: R=%d beyond %d", R, IVEC_MAX_R);
  return fgmm_launch_tv_planes(T, icov, G, Pk, C, D, R, (hipStream_t)stream);
}
