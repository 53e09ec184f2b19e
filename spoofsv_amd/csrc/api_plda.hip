// C-ABI entries of the i-vector back end (include/ssv_hip.h, "I-vector back end: PLDA"): the argument checks, which come before any launch
// and need no device; the kernels are in plda.hip, the product of the transform in ivector_tv.hip, the rank limit and the launchers'
// declarations in ivec_chain.h.
#include "ssv_host.h"
#include "ivec_chain.h"

static int plda_rank(const char* what, int R) {
  SSV_CHECK(R >= 1, SSV_BAD_SHAPE, "%s: need R >= 1; got R=%d", what, R);
  SSV_CHECK(R <= IVEC_MAX_R, SSV_UNSUPPORTED, "%s: R=%d (at most %d) beyond the kernels", what, R, IVEC_MAX_R);
  return 0;
}

extern "C" int ssv_plda_class_stats(const float* X, const long* spk_off, const long* spk_off_host, float* Xd, double* means, double* mu, float* model, long n,
                                    int S, int R, int length_norm, ssv_stream_t stream) {
  SSV_CHECK(X && spk_off, SSV_BAD_SHAPE, "plda_class_stats: null pointer (X and spk_off are required)");
  SSV_CHECK(Xd || means || model, SSV_BAD_SHAPE, "plda_class_stats: null outputs (one of Xd, means and model is required)");
  SSV_CHECK(!mu || means, SSV_BAD_SHAPE, "plda_class_stats: mu is the mean of the means: means is required with it");
  SSV_CHECK(n >= 1 && S >= 1, SSV_BAD_SHAPE, "plda_class_stats: need n >= 1 and S >= 1; got n=%ld S=%d", n, S);
  SSV_TRY(plda_rank("plda_class_stats", R));
  SSV_TRY(host_offsets_ok("plda_class_stats", "spk_off", "speaker", "rows", spk_off_host, S, n));
  return plda_launch_class_stats(X, spk_off, Xd, means, mu, model, n, S, R, length_norm != 0, (hipStream_t)stream);
}

extern "C" int ssv_plda_mixed_inverse(const double* a, const double* b, long b_stride, const double* coef, double* out, double* logdet, int J, int R,
                                      ssv_stream_t stream) {
  SSV_CHECK(b && out, SSV_BAD_SHAPE, "plda_mixed_inverse: null pointer (b and out are required; a, coef and logdet are optional)");
  SSV_CHECK(J >= 1 && b_stride >= 0, SSV_BAD_SHAPE, "plda_mixed_inverse: need J >= 1 and b_stride >= 0; got J=%d b_stride=%ld", J, b_stride);
  SSV_TRY(plda_rank("plda_mixed_inverse", R));
  return plda_launch_mixed_inverse(a, b, b_stride, coef, out, logdet, J, R, (hipStream_t)stream);
}

extern "C" int ssv_plda_em_classes(const double* means, const double* mu, const int* cnt, const int* cls, const double* Mx, const double* Winv, double* w, double* r,
                                   double* quad, int S, int J, int R, ssv_stream_t stream) {
  SSV_CHECK(means && mu && cnt && cls && Mx && Winv, SSV_BAD_SHAPE, "plda_em_classes: null pointer (means, mu, cnt, cls, Mx and Winv are required)");
  SSV_CHECK(w && r && quad, SSV_BAD_SHAPE, "plda_em_classes: null outputs (w, r and quad are required)");
  SSV_CHECK(S >= 1 && J >= 1, SSV_BAD_SHAPE, "plda_em_classes: need S >= 1 and J >= 1; got S=%d J=%d", S, J);
  SSV_TRY(plda_rank("plda_em_classes", R));
  return plda_launch_em_classes(means, mu, cnt, cls, Mx, Winv, w, r, quad, S, R, J, (hipStream_t)stream);
}

extern "C" int ssv_plda_wsyrk_f64(const double* V, const double* c, double* acc, long S, int R, ssv_stream_t stream) {
  SSV_CHECK(V, SSV_BAD_SHAPE, "plda_wsyrk_f64: null pointer (V is required; c is optional)");
  SSV_CHECK(acc, SSV_BAD_SHAPE, "plda_wsyrk_f64: null output (acc is required)");
  SSV_CHECK(S >= 1, SSV_BAD_SHAPE, "plda_wsyrk_f64: need S >= 1; got S=%ld", S);
  SSV_TRY(plda_rank("plda_wsyrk_f64", R));
  return plda_launch_wsyrk(V, c, acc, S, R, (hipStream_t)stream);
}

extern "C" int ssv_plda_em_update(const double* Mx, const double* ldMx, const double* nspk, const double* nrow, const double* WW, const double* RR,
                                  const double* Sigma, const double* Winv, const double* ldW, const double* ldB, const int* cnt, const int* cls, const double* quad,
                                  double* W, double* B, double* obj, int J, int S, int R, double Sn, double N, ssv_stream_t stream) {
  SSV_CHECK((W != nullptr) == (B != nullptr) && (W || obj), SSV_BAD_SHAPE, "plda_em_update: null outputs (W and B together, obj, or all three)");
  SSV_CHECK(Sigma, SSV_BAD_SHAPE, "plda_em_update: null pointer (Sigma is required)");
  SSV_CHECK(!W || (Mx && nspk && nrow && WW && RR), SSV_BAD_SHAPE, "plda_em_update: null pointer (the update needs Mx, nspk, nrow, WW and RR)");
  SSV_CHECK(!obj || (ldMx && Winv && ldW && ldB && cnt && cls && quad), SSV_BAD_SHAPE,
            "plda_em_update: null pointer (the objective needs ldMx, Winv, ldW, ldB, cnt, cls and quad)");
  SSV_CHECK(J >= 1 && S >= 1 && Sn >= 1.0 && N >= Sn, SSV_BAD_SHAPE, "plda_em_update: need J >= 1, S >= 1 and 1 <= Sn <= N; got J=%d S=%d Sn=%g N=%g", J, S, Sn, N);
  SSV_TRY(plda_rank("plda_em_update", R));
  return plda_launch_em_update(Mx, ldMx, nspk, nrow, WW, RR, Sigma, Winv, ldW, ldB, cnt, cls, quad, W, B, obj, J, S, R, Sn, N, (hipStream_t)stream);
}

extern "C" int ssv_plda_transform(const float* X, const double* mu, const float* At, const double* psi, const int* nex, int nex_all, float* Xc, float* U, long n, int R,
                                  int length_norm, ssv_stream_t stream) {
  SSV_CHECK(X && mu && At && psi, SSV_BAD_SHAPE, "plda_transform: null pointer (X, mu, At and psi are required)");
  SSV_CHECK(Xc && U && Xc != U && Xc != X, SSV_BAD_SHAPE, "plda_transform: null outputs (the workspace Xc and U are required, apart from each other and from X)");
  SSV_CHECK(n >= 1 && (nex || nex_all >= 1), SSV_BAD_SHAPE, "plda_transform: need n >= 1 and, without nex, nex_all >= 1; got n=%ld nex_all=%d", n, nex_all);
  SSV_TRY(plda_rank("plda_transform", R));
  SSV_TRY(plda_launch_centre(X, mu, Xc, n, R, length_norm != 0, (hipStream_t)stream));
  SSV_TRY(tv_launch_product(Xc, At, U, n, R, R, (hipStream_t)stream));
  return plda_launch_scale(U, psi, nex, nex_all, n, R, (hipStream_t)stream);
}

extern "C" int ssv_plda_speaker_planes(const float* y, const int* nspk, const double* psi, float* H, double* k, int S, int R, ssv_stream_t stream) {
  SSV_CHECK(y && nspk && psi, SSV_BAD_SHAPE, "plda_speaker_planes: null pointer (y, nspk and psi are required)");
  SSV_CHECK(H && k, SSV_BAD_SHAPE, "plda_speaker_planes: null outputs (H and k are required)");
  SSV_CHECK(S >= 1, SSV_BAD_SHAPE, "plda_speaker_planes: need S >= 1; got S=%d", S);
  SSV_TRY(plda_rank("plda_speaker_planes", R));
  return plda_launch_speaker_planes(y, nspk, psi, H, k, S, R, (hipStream_t)stream);
}

extern "C" int ssv_plda_score(const float* T, const float* H, const double* k, float* scores, long E, long S, int R, ssv_stream_t stream) {
  SSV_CHECK(T && H && k, SSV_BAD_SHAPE, "plda_score: null pointer (T, H and k are required)");
  SSV_CHECK(scores, SSV_BAD_SHAPE, "plda_score: null output (scores is required)");
  SSV_CHECK(E >= 1 && S >= 1, SSV_BAD_SHAPE, "plda_score: need E >= 1 and S >= 1; got E=%ld S=%ld", E, S);
  SSV_TRY(plda_rank("plda_score", R));
  return plda_launch_score(T, H, k, scores, E, S, R, (hipStream_t)stream);
}
