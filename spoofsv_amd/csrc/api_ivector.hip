// C-ABI entries of the i-vector front half (include/ssv_hip.h, "I-vector groundwork"): the argument checks, which come before any launch
// and need no device; the kernels are in ivector.hip, the limits and the launchers' declarations in ivec_chain.h.
#include "ssv_host.h"
#include "ivec_chain.h"
#include "exact_product.h"        // XP_RUN, XP_TILE

extern "C" long ssv_ivec_features_workspace(long G, int Cc, int delta_order) {
  if (G < 1 || Cc < 1 || delta_order < 0 || delta_order > 2) return 0;
  return (long)align256((size_t)G * Cc * (delta_order + 1) * sizeof(float));
}

extern "C" int ssv_ivec_features(const float* mel, const long* utt_off, const float* dct, float* out, long G, int M, int U, int Cc, int delta_window,
                                 int delta_order, int cmn_window, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(mel && utt_off && out && ws, SSV_BAD_SHAPE, "ivec_features: null pointer (mel, utt_off, out and ws are required)");
  SSV_CHECK(G >= 1 && M >= 1 && U >= 1 && Cc >= 1 && cmn_window >= 1, SSV_BAD_SHAPE, "ivec_features: need G >= 1, M >= 1, U >= 1, Cc >= 1 and cmn_window >= 1; got G=%ld M=%d U=%d Cc=%d cmn_window=%d",
            G, M, U, Cc, cmn_window);
  SSV_CHECK(delta_order >= 0 && delta_order <= 2 && (delta_order == 0 || delta_window >= 1), SSV_BAD_SHAPE,
            "ivec_features: delta_order=%d must be 0, 1 or 2 and delta_window=%d >= 1 when deltas are asked for", delta_order, delta_window);
  SSV_CHECK(dct || Cc == M, SSV_BAD_SHAPE, "ivec_features: without a dct table the statics are the mel frames themselves: Cc=%d must equal M=%d", Cc, M);
  SSV_CHECK(ws_bytes >= (size_t)ssv_ivec_features_workspace(G, Cc, delta_order), SSV_BAD_SHAPE, "ivec_features: workspace of %zu bytes, %ld needed", ws_bytes,
            ssv_ivec_features_workspace(G, Cc, delta_order));
  return ivec_launch_features(mel, utt_off, dct, out, (float*)ws, G, M, U, Cc, delta_order, delta_window, cmn_window, (hipStream_t)stream);
}

extern "C" int ssv_gmm_frame_tile(int D, int C) {
  SSV_CHECK(D >= 1 && C >= 1, SSV_BAD_SHAPE, "gmm_frame_tile: need D >= 1 and C >= 1; got D=%d C=%d", D, C);
  const int tf = ivec_gselect_tile(D, C, nullptr);
  SSV_CHECK(tf > 0, SSV_UNSUPPORTED, "gmm_frame_tile: D=%d, C=%d are beyond the tiles", D, C);
  return tf;
}

extern "C" int ssv_gmm_diag_gselect(const float* X, const float* A, const float* B, const float* g, int* idx, float* post, float* loglik, long F, int D, int C,
                                    int nsel, float min_post, ssv_stream_t stream) {
  SSV_CHECK(X && A && B && g && idx && post && loglik, SSV_BAD_SHAPE, "gmm_diag_gselect: null pointer (X, A, B, g, idx, post and loglik are required)");
  SSV_CHECK(F >= 1 && D >= 1 && C >= 1 && nsel >= 1 && nsel <= C, SSV_BAD_SHAPE, "gmm_diag_gselect: need F >= 1, D >= 1 and 1 <= nsel <= C; got F=%ld D=%d C=%d nsel=%d", F,
            D, C, nsel);
  SSV_CHECK(min_post >= 0.f && min_post < 1.f, SSV_BAD_SHAPE, "gmm_diag_gselect: min_post=%g must lie in [0, 1)", (double)min_post);
  SSV_CHECK((D & 3) != 0 || (((uintptr_t)A | (uintptr_t)B) & 15) == 0, SSV_BAD_SHAPE, "gmm_diag_gselect: with D %% 4 == 0 the planes A and B must be 16-byte aligned");
  return ivec_launch_gselect(X, A, B, g, idx, post, loglik, F, D, C, nsel, min_post, (hipStream_t)stream);
}

extern "C" int ssv_gmm_diag_stats(const float* X, const int* idx, const float* post, const long* seg_off, const long* seg_off_host, float* slab, long F, int D,
                                  int C, int nsel, int S, int order, ssv_stream_t stream) {
  SSV_CHECK(X && idx && post && seg_off && slab, SSV_BAD_SHAPE, "gmm_diag_stats: null pointer (X, idx, post, seg_off and slab are required)");
  SSV_CHECK(F >= 1 && D >= 1 && C >= 1 && nsel >= 1 && nsel <= C && S >= 1, SSV_BAD_SHAPE,
            "gmm_diag_stats: need F >= 1, D >= 1, 1 <= nsel <= C and S >= 1; got F=%ld D=%d C=%d nsel=%d S=%d", F, D, C, nsel, S);
  SSV_CHECK(order == 1 || order == 2, SSV_BAD_SHAPE, "gmm_diag_stats: order=%d must be 1 or 2", order);
  SSV_TRY(host_offsets_ok("gmm_diag_stats", "seg_off", "segment", "frames", seg_off_host, S, F));
  return ivec_launch_stats(X, idx, post, seg_off, slab, F, D, C, nsel, S, order, (hipStream_t)stream);
}

extern "C" int ssv_gmm_stats_reduce(const float* slab, double* out, int S, long n, ssv_stream_t stream) {
  SSV_CHECK(slab && out, SSV_BAD_SHAPE, "gmm_stats_reduce: null pointer (slab and out are required)");
  SSV_CHECK(S >= 1 && n >= 1, SSV_BAD_SHAPE, "gmm_stats_reduce: need S >= 1 and n >= 1; got S=%d n=%ld", S, n);
  SSV_CHECK((n + 255) / 256 <= 0x7fffffffL, SSV_UNSUPPORTED, "gmm_stats_reduce: n=%ld exceeds the grid", n);
  return ivec_launch_reduce(slab, out, S, n, (hipStream_t)stream);
}

static int gmm_cd_ok(const char* what, int C, int D) {
  SSV_CHECK(C >= 1 && D >= 1, SSV_BAD_SHAPE, "%s: need C >= 1 and D >= 1; got C=%d D=%d", what, C, D);
  SSV_CHECK(C <= IVEC_MAX_C && D <= IVEC_MAX_D, SSV_UNSUPPORTED, "%s: C=%d (at most %d) or D=%d (at most %d) beyond what the other entries take", what, C, IVEC_MAX_C, D,
            IVEC_MAX_D);
  return 0;
}

extern "C" int ssv_gmm_diag_update(const double* stats, double* w, double* mu, double* var, float* A, float* B, float* g, int C, int D, double var_floor,
                                   double min_count, double min_weight, ssv_stream_t stream) {
  SSV_CHECK(stats && w && mu && var && A && B && g, SSV_BAD_SHAPE, "gmm_diag_update: null pointer (stats, w, mu, var, A, B and g are required)");
  SSV_TRY(gmm_cd_ok("gmm_diag_update", C, D));
  SSV_CHECK(var_floor > 0.0 && min_weight > 0.0 && min_weight < 1.0 && min_count >= 0.0, SSV_BAD_SHAPE,
            "gmm_diag_update: need var_floor > 0, min_count >= 0 and 0 < min_weight < 1; got %g, %g, %g", var_floor, min_count, min_weight);
  return ivec_launch_update(stats, nullptr, w, mu, var, A, B, g, C, D, var_floor, min_count, min_weight, (hipStream_t)stream);
}

extern "C" int ssv_gmm_diag_planes(const double* w, const double* mu, const double* var, float* A, float* B, float* g, int C, int D, ssv_stream_t stream) {
  SSV_CHECK(w && mu && var && A && B && g, SSV_BAD_SHAPE, "gmm_diag_planes: null pointer (w, mu, var, A, B and g are required)");
  SSV_TRY(gmm_cd_ok("gmm_diag_planes", C, D));
  return ivec_launch_update(nullptr, w, nullptr, (double*)mu, (double*)var, A, B, g, C, D, 1.0, 0.0, 0.5, (hipStream_t)stream);
}

// ---- the i-vector extractor (include/ssv_hip.h, "I-vector extractor"): kernels in ivector_tv.hip ------------------------------------------
extern "C" int ssv_ivec_tv_planes(const double* T, const double* var, float* G, float* Pk, int C, int D, int R, ssv_stream_t stream) {
  SSV_CHECK(T && var && G && Pk, SSV_BAD_SHAPE, "ivec_tv_planes: null pointer (T, var, G and Pk are required)");
  SSV_CHECK(C >= 1 && D >= 1 && R >= 1, SSV_BAD_SHAPE, "ivec_tv_planes: need C >= 1, D >= 1 and R >= 1; got C=%d D=%d R=%d", C, D, R);
  return tv_launch_planes(T, var, G, Pk, C, D, R, (hipStream_t)stream);
}

extern "C" int ssv_ivec_centre_stats(const float* N, const float* F, const double* mu, float* Ft, long U, int C, int D, ssv_stream_t stream) {
  SSV_CHECK(N && F && mu && Ft, SSV_BAD_SHAPE, "ivec_centre_stats: null pointer (N, F, mu and Ft are required)");
  SSV_CHECK(U >= 1 && C >= 1 && D >= 1, SSV_BAD_SHAPE, "ivec_centre_stats: need U >= 1, C >= 1 and D >= 1; got U=%ld C=%d D=%d", U, C, D);
  return tv_launch_centre(N, F, mu, Ft, U, C, D, (hipStream_t)stream);
}

extern "C" int ssv_ivec_product_run(void) { return XP_RUN; }
extern "C" int ssv_ivec_product_tile(void) { return XP_TILE; }

extern "C" int ssv_ivec_product(const float* A, const float* B, float* out, long m, long n, long K, ssv_stream_t stream) {
  SSV_CHECK(A && B && out, SSV_BAD_SHAPE, "ivec_product: null pointer (A, B and out are required)");
  SSV_CHECK(m >= 1 && n >= 1 && K >= 1, SSV_BAD_SHAPE, "ivec_product: need m >= 1, n >= 1 and K >= 1; got m=%ld n=%ld K=%ld", m, n, K);
  return tv_launch_product(A, B, out, m, n, K, (hipStream_t)stream);
}

extern "C" int ssv_ivec_product_tn(const float* A, const float* B, double* acc, long U, long m, long n, ssv_stream_t stream) {
  SSV_CHECK(A && B && acc, SSV_BAD_SHAPE, "ivec_product_tn: null pointer (A, B and acc are required)");
  SSV_CHECK(U >= 1 && m >= 1 && n >= 1, SSV_BAD_SHAPE, "ivec_product_tn: need U >= 1, m >= 1 and n >= 1; got U=%ld m=%ld n=%ld", U, m, n);
  return tv_launch_product_tn(A, B, acc, U, m, n, (hipStream_t)stream);
}

extern "C" int ssv_ivec_estep(const float* Lp, const float* b, float* w, float* M, double* obj, long U, int R, ssv_stream_t stream) {
  SSV_CHECK(Lp && b && w && obj, SSV_BAD_SHAPE, "ivec_estep: null pointer (Lp, b, w and obj are required; M is optional)");
  SSV_CHECK(U >= 1 && R >= 1, SSV_BAD_SHAPE, "ivec_estep: need U >= 1 and R >= 1; got U=%ld R=%d", U, R);
  return tv_launch_estep(Lp, b, w, M, obj, U, R, (hipStream_t)stream);
}

extern "C" int ssv_ivec_tv_update(const double* A, const double* Cm, const double* Nc, const double* J, double* T, int C, int D, int R, double min_count,
                                  ssv_stream_t stream) {
  SSV_CHECK(A && Cm && Nc && T, SSV_BAD_SHAPE, "ivec_tv_update: null pointer (A, Cm, Nc and T are required; J is optional)");
  SSV_CHECK(C >= 1 && D >= 1 && R >= 1 && min_count >= 0.0, SSV_BAD_SHAPE, "ivec_tv_update: need C >= 1, D >= 1, R >= 1 and min_count >= 0; got C=%d D=%d R=%d min_count=%g",
            C, D, R, min_count);
  return tv_launch_update(A, Cm, Nc, J, T, C, D, R, min_count, (hipStream_t)stream);
}

extern "C" int ssv_ivec_cosine_trials(const float* enroll, const long* spk_off, const long* spk_off_host, const float* evalv, float* scores, long n_enroll, int S,
                                      long E, int R, ssv_stream_t stream) {
  SSV_CHECK(enroll && spk_off && evalv && scores, SSV_BAD_SHAPE, "ivec_cosine_trials: null pointer (enroll, spk_off, evalv and scores are required)");
  SSV_CHECK(n_enroll >= 1 && S >= 1 && E >= 1 && R >= 1, SSV_BAD_SHAPE, "ivec_cosine_trials: need n_enroll >= 1, S >= 1, E >= 1 and R >= 1; got n_enroll=%ld S=%d E=%ld R=%d",
            n_enroll, S, E, R);
  SSV_TRY(host_offsets_ok("ivec_cosine_trials", "spk_off", "speaker", "enrolment vectors", spk_off_host, S, n_enroll));
  return tv_launch_cosine(enroll, spk_off, evalv, scores, n_enroll, S, E, R, (hipStream_t)stream);
}
