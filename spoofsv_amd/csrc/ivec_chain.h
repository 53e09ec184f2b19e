// Internal header of the i-vector chain (ivector.hip, ivector_tv.hip, plda.hip, fgmm.hip and their api_*.hip files): the shape limits
// every stage shares and the ONE declaration of each launcher, seen by the file that defines it and by the files that call it.
// No kernel, no entry point.  (spoofsv_amd/ivector.py states the limits once more for its own messages.)
#pragma once
#include "ssv_common.h"

#define IVEC_MAX_C 2048             // Gaussians of a mixture
#define IVEC_MAX_D 128              // feature dimension
#define IVEC_MAX_NSEL 32            // Gaussians selected per frame
#define IVEC_MAX_R 192              // rank: the packed float64 triangle of R = 192 is 148,224 bytes, it fits the 160 KiB LDS with the vectors
#define FGMM_TILE 64                // full-covariance UBM: pairs one workgroup of the product kernels owns per step (ssv_fgmm_pair_tile)
#define FGMM_SL 4096                // full-covariance UBM: slots per workgroup of the counting sort

#pragma GCC visibility push(hidden)      // the launchers: shared between the chain's files, not exported
// ---- ivector.hip
int ivec_launch_features(const float* mel, const long* utt_off, const float* dct, float* out, float* v, long G, int M, int U, int Cc, int order, int w, int W,
                         hipStream_t st);
int ivec_gselect_tile(int D, int C, size_t* lds_bytes);      // frames per workgroup, 0 = beyond the tiles
int ivec_launch_gselect(const float* X, const float* A, const float* B, const float* g, int* idx, float* post, float* loglik, long F, int D, int C, int nsel,
                        float min_post, hipStream_t st);
int ivec_launch_stats(const float* X, const int* idx, const float* post, const long* seg_off, float* slab, long F, int D, int C, int nsel, int S, int order,
                      hipStream_t st);
int ivec_launch_reduce(const float* slab, double* out, int S, long n, hipStream_t st);
int ivec_launch_update(const double* stats, const double* w_in, double* w_out, double* mu, double* var, float* A, float* B, float* g, int C, int D,
                       double var_floor, double min_count, double min_weight, hipStream_t st);
// ---- ivector_tv.hip
int tv_launch_planes(const double* T, const double* var, float* G, float* Pk, int C, int D, int R, hipStream_t st);
int tv_launch_centre(const float* N, const float* F, const double* mu, float* Ft, long U, int C, int D, hipStream_t st);
int tv_launch_product(const float* A, const float* B, float* out, long m, long n, long K, hipStream_t st);
int tv_launch_product_tn(const float* A, const float* B, double* acc, long U, long m, long n, hipStream_t st);
int tv_launch_estep(const float* Lp, const float* b, float* w, float* M, double* obj, long U, int R, hipStream_t st);
int tv_launch_update(const double* A, const double* Cm, const double* Nc, const double* J, double* T, int C, int D, int R, double min_count, hipStream_t st);
int tv_launch_cosine(const float* enroll, const long* spk_off, const float* evalv, float* scores, long n_enroll, int S, long E, int R, hipStream_t st);
// ---- plda.hip
int plda_launch_class_stats(const float* X, const long* spk_off, float* Xd, double* means, double* mu, float* model, long n, int S, int R, int length_norm,
                            hipStream_t st);
int plda_launch_mixed_inverse(const double* a, const double* b, long b_stride, const double* coef, double* out, double* logdet, int J, int R, hipStream_t st);
int plda_launch_em_classes(const double* means, const double* mu, const int* cnt, const int* cls, const double* Mx, const double* Winv, double* w, double* r,
                           double* quad, int S, int R, int J, hipStream_t st);
int plda_launch_wsyrk(const double* V, const double* c, double* acc, long S, int R, hipStream_t st);
int plda_launch_em_update(const double* Mx, const double* ldMx, const double* nspk, const double* nrow, const double* WW, const double* RR, const double* Sigma,
                          const double* Winv, const double* ldW, const double* ldB, const int* cnt, const int* cls, const double* quad, double* W, double* B,
                          double* obj, int J, int S, int R, double Sn, double N, hipStream_t st);
int plda_launch_centre(const float* X, const double* mu, float* Xc, long n, int R, int length_norm, hipStream_t st);
int plda_launch_scale(float* U, const double* psi, const int* nex, int nex_all, long n, int R, hipStream_t st);
int plda_launch_speaker_planes(const float* y, const int* nspk, const double* psi, float* H, double* k, int S, int R, hipStream_t st);
int plda_launch_score(const float* T, const float* H, const double* k, float* scores, long E, long S, int R, hipStream_t st);
// ---- fgmm.hip
int fgmm_launch_planes(const double* w, const double* mu, const double* cov, float* Wt, float* muf, float* g, double* icov, int C, int D, hipStream_t st);
int fgmm_launch_group(const int* idx, int* start, int* pairs, int* counts, long n, int C, hipStream_t st);
int fgmm_launch_post(const float* X, const float* Wt, const float* muf, const float* g, const int* idx, const int* start, const int* pairs, float* post,
                     float* loglik, float* L, long F, int D, int C, int nsel, int nrun, float min_post, hipStream_t st);
int fgmm_launch_stats(const float* X, const float* muf, const float* post, const int* start, const int* pairs, float* slab, long F, int D, int C, int nsel,
                      int nrun, hipStream_t st);
int fgmm_launch_update(const double* stats, double* w, double* mu, double* cov, float* Wt, float* muf, float* g, double* icov, int* kept, int C, int D,
                       double var_floor, double min_count, double min_weight, hipStream_t st);
int fgmm_launch_tv_planes(const double* T, const double* icov, float* G, float* Pk, int C, int D, int R, hipStream_t st);
#pragma GCC visibility pop
