// kernels_timer.inc — part of kernels.hip's translation unit (not compiled on its own).
// Host code: KernelTimer (kernels.hpp) and the DINO_SYNC_CHECK switch; needs nothing from what stands before it.
void KernelTimer::begin(int k, hipStream_t s) {
  if (!enabled) return;
  if (!created) {
    for (int i = 0; i < kMaxPending; ++i) {
      (void)hipEventCreate(&ev[i][0]);
      (void)hipEventCreate(&ev[i][1]);
    }
    created = true;
    reset();
  }
  if (n >= kMaxPending) collect();
  id[n] = k;
  (void)hipEventRecord(ev[n][0], s);
}

void KernelTimer::end(hipStream_t s) {
  if (!enabled || !created) return;
  (void)hipEventRecord(ev[n][1], s);
  ++n;
}

void KernelTimer::collect() {
  for (int i = 0; i < n; ++i) {
    float ms = 0.f;
    (void)hipEventSynchronize(ev[i][1]);
    if (hipEventElapsedTime(&ms, ev[i][0], ev[i][1]) == hipSuccess) {
      total_ms[id[i]] += ms;
      count[id[i]] += 1;
    }
  }
  n = 0;
}

void KernelTimer::reset() {
  n = 0;
  for (int i = 0; i < kKNumKernels; ++i) {
    total_ms[i] = 0.0;
    count[i] = 0;
  }
}

void KernelTimer::destroy() {
  if (!created) return;
  for (int i = 0; i < kMaxPending; ++i) {
    (void)hipEventDestroy(ev[i][0]);
    (void)hipEventDestroy(ev[i][1]);
  }
  created = false;
}

// DINO_SYNC_CHECK=1: synchronise after every kernel and report which one failed
// (debugging aid; pinpoints a faulting kernel instead of a later sync point).
static const bool g_sync_check = [] {
  const char* v = getenv("DINO_SYNC_CHECK");
  return v && v[0] == '1';
}();
