// Body of dtw_error_kernel<LEN> and dtw_error_signals_kernel<LEN> (scoring.hip), included after each kernel's prologue: the loop
// over the timesteps of one series -- the whole series, or the segment the workgroup took from blockIdx.y.
// Expects from the enclosing scope: y, yh (the series), out (its output), T (its timesteps), LEN and HALF = LEN / 2.
// Shared as text, not as a function: see the note at unroll_median_signals_kernel.
  for (int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x; p < T; p += (int64_t)gridDim.x * THREADS) {
    const int64_t i = p - HALF;                 // window start in padded coordinates
    if (i < 0 || i >= T - LEN) { out[p] = 0.0; continue; }
    double a[LEN], b[LEN], row[LEN];
#pragma unroll
    for (int k = 0; k < LEN; ++k) {
      int64_t src = i + k - HALF;               // y_pad[i + k] = y[i + k - HALF]
      bool ok = src >= 0 && src < T;
      a[k] = ok ? y[src] : 0.0;
      b[k] = ok ? (double)yh[src] : 0.0;
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LEN; ++j) { double d = a[0] - b[j]; acc += d * d; row[j] = acc; }
#pragma unroll
    for (int r = 1; r < LEN; ++r) {
      double diag = row[0];
      double d0 = a[r] - b[0];
      row[0] = row[0] + d0 * d0;
#pragma unroll
      for (int j = 1; j < LEN; ++j) {
        double up = row[j];
        double d = a[r] - b[j];
        double m = fmin(fmin(up, row[j - 1]), diag);
        row[j] = d * d + m;
        diag = up;
      }
    }
    out[p] = sqrt(row[LEN - 1]);
  }
