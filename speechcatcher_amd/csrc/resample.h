// Sample-rate conversion (resample.hip): what the stream engine (streams.hip) shares with the kernel's launcher.
#pragma once
#include "common.h"

constexpr int SC_RS_MAX_TABS = 8;    // distinct input rates per sc_streams
constexpr int SC_RS_HIST = 160;      // floats per history row (K - 1 <= 153 are used)

// coefficient tables a launch can name: [L][2 Wc] f32 on the device
struct sc_rs_tabs {
  const float *coef[SC_RS_MAX_TABS];
  int32_t L[SC_RS_MAX_TABS], M[SC_RS_MAX_TABS], Wc[SC_RS_MAX_TABS];
};

// one stream's call: n_in staged samples at src + src_off behind the n_before samples the stream has taken -> the n_out
// outputs m0 .. m0 + n_out - 1 at dst + dst_off.  The history is read from row `par` of the stream, written to 1 - par.
struct sc_rs_job {
  long long src_off, n_in, dst_off, n_out, m0, n_before;
  int32_t tab, stream, par, pad;
};

// L, M, half width of the design for `rate`; false: unsupported
bool sc_rs_params(int rate, int *L, int *M, int *Wc);
// outputs after n_in_total input samples (is_final: after the flush)
long sc_rs_out_count(int L, int M, int Wc, long n_in_total, bool is_final);
// workgroups along x that a job of n_out outputs over table `tab` needs (the tile is 256 outputs for L <= 4, else 4 L)
long long sc_rs_tiles(const sc_rs_tabs &tabs, int tab, long long n_out);
// one launch for n_jobs jobs (jobs_dev, or the single job *one passed by value); tiles: the largest sc_rs_tiles among them.
// hist [2][S][SC_RS_HIST] or NULL (no history is read or left: a whole signal at once)
int sc_rs_launch(const sc_rs_tabs &tabs, const sc_rs_job *one, const sc_rs_job *jobs_dev, int n_jobs, long long tiles,
                 const float *src, float *dst, float *hist, int S, hipStream_t st);
