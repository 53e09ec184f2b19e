// extern "C" entry points of libssv_hip.so (see include/ssv_hip.h): argument checking and the
// composition of kernel launches for each replaced module of the reference.  No allocation, no
// synchronisation: everything is enqueued on the caller's stream.
// This file: what every module shares at run time -- the error state, the arithmetic mode, the tuning knobs, the shape log and the
// version entries.  The modules' entry points: api_conv.hip (convolutions, resident weight planes, transposed convolution),
// api_norm.hip (LayerNorm, 1x1 links, highway blocks, second order), api_attn.hip, api_lstm.hip and api_lstm_train.hip (GE2E);
// what they share at compile time is ssv_host.h.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssv_common.h"

// ---- error state ---------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
int ssv_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int ssv_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  ssv_fail(0, "%s: launch failed: %s", what, hipGetErrorString(e));
  return -(int)e;
}
static int g_precision = -1;
// SSV_PRECISION, strictly parsed: -> 0 | 1 | 2, or -1 when the variable names no mode (a typo must not silently select another arithmetic)
static int precision_from_env() {
  const char* e = getenv("SSV_PRECISION");
  if (!e || !*e || !strcmp(e, "f16x2") || !strcmp(e, "2")) return 2;
  if (!strcmp(e, "fp32") || !strcmp(e, "0")) return 0;
  if (!strcmp(e, "bf16x3") || !strcmp(e, "1")) return 1;
  return -1;
}
int ssv_precision() {
  if (g_precision < 0) {
    g_precision = precision_from_env();
    if (g_precision < 0) {
      // Reached only by a host that neither asked ssv_get_precision() (which reports the bad value as an error) nor chose a mode with
      // ssv_set_precision() before its first compute call: no arithmetic at all rather than another one than was asked for.
      fprintf(stderr, "libssv_hip: SSV_PRECISION=%s is not one of fp32|0, bf16x3|1, f16x2|2 (call ssv_set_precision to choose a mode)\n", getenv("SSV_PRECISION"));
      abort();
    }
  }
  return g_precision;
}
static const char* const g_knob_names[SSV_T_COUNT] = {"SSV_NT_FORCE", "SSV_NNB_FORCE", "SSV_LN_GROUPS", "SSV_LN_PERSIST", "SSV_LSTM_MERGE", "SSV_PWLN_BWD"};
static char g_knob_val[SSV_T_COUNT][512];
static const char* g_knob[SSV_T_COUNT];
static int g_knobs_loaded = 0;
static void load_knobs() {
  for (int i = 0; i < SSV_T_COUNT; ++i) {
    const char* e = getenv(g_knob_names[i]);
    if (e) { strncpy(g_knob_val[i], e, sizeof g_knob_val[i] - 1); g_knob_val[i][sizeof g_knob_val[i] - 1] = 0; g_knob[i] = g_knob_val[i]; }
    else g_knob[i] = nullptr;
  }
  __atomic_store_n(&g_knobs_loaded, 1, __ATOMIC_RELEASE);
}
const char* ssv_tuning(int knob) {
  if (!__atomic_load_n(&g_knobs_loaded, __ATOMIC_ACQUIRE)) load_knobs();
  return g_knob[knob];
}
extern "C" void ssv_reload_tuning(void) { load_knobs(); }
// ---- shape log (see ssv_common.h) ---------------------------------------------------------------
#include <mutex>
#include <string>
#include <map>
static int g_shape_log = -1;
static std::string g_shape_path;                                 // cached when the log is enabled: the environment may change before exit
static std::mutex g_shape_mu;
static std::map<std::string, long>* g_shape_seen = nullptr;      // line -> host-side launches (eager and capture passes; replays do not come here)
static void shape_log_flush() {
  std::lock_guard<std::mutex> lk(g_shape_mu);
  if (!g_shape_seen) return;
  if (g_shape_path.empty()) return;
  if (FILE* f = fopen(g_shape_path.c_str(), "w")) {
    for (const auto& kv : *g_shape_seen) fprintf(f, "%s\t%ld\n", kv.first.c_str(), kv.second);
    fclose(f);
  }
}
bool ssv_shape_log_on() {
  if (g_shape_log < 0) { const char* e = getenv("SSV_SHAPE_LOG"); g_shape_log = (e && *e) ? 1 : 0; if (g_shape_log) { g_shape_path = e; atexit(shape_log_flush); } }
  return g_shape_log == 1;
}
void ssv_shape_log(const char* kernel, dim3 grid, dim3 block, double flops, double bytes, const char* note) {
  if (!ssv_shape_log_on()) return;
  char line[768];
  snprintf(line, sizeof line, "%s\t%ux%ux%u\t%.6g\t%.6g\t%s", kernel, grid.x * block.x, grid.y * block.y, grid.z * block.z, flops, bytes, note ? note : "");
  std::lock_guard<std::mutex> lk(g_shape_mu);
  if (!g_shape_seen) g_shape_seen = new std::map<std::string, long>();
  ++(*g_shape_seen)[line];
}
// An unknown SSV_PRECISION value is an ERROR of these two entries (SSV_UNSUPPORTED + ssv_last_error), not the end of the process: a C host
// that asks for the mode first, or sets one explicitly (which overrides the variable), never reaches the abort in ssv_precision().
extern "C" int ssv_set_precision(int mode) {
  int prev = g_precision >= 0 ? g_precision : precision_from_env();
  if (prev < 0) prev = ssv_fail(SSV_UNSUPPORTED, "SSV_PRECISION=%s is not one of fp32|0, bf16x3|1, f16x2|2; mode %d set explicitly", getenv("SSV_PRECISION"), mode);
  g_precision = mode <= 0 ? 0 : (mode == 1 ? 1 : 2);
  return prev;
}
extern "C" int ssv_get_precision(void) {
  if (g_precision < 0 && precision_from_env() < 0)
    return ssv_fail(SSV_UNSUPPORTED, "SSV_PRECISION=%s is not one of fp32|0, bf16x3|1, f16x2|2", getenv("SSV_PRECISION"));
  return ssv_precision();
}
extern "C" int ssv_version(void) { return 7; }
extern "C" const char* ssv_arch(void) { return "gfx950"; }
extern "C" const char* ssv_last_error(void) { return g_err; }
