// scan_kernels.hpp — the generic segment scan (scan_kernels.hip) and its
// scratch, one per engine (E.scan): every device call that needs per-key
// offsets scans through it, on the engine's stream, one scan after another.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace ccrdt {

struct ScanScratch {
  hipStream_t stream = nullptr;  // the engine's: every scan is queued there, so the scans share the scratch in order
  // Room for a scan over n elements.  Growing waits for the device: a call
  // that must not wait between its passes asks before its first launch.
  int ensure(uint64_t n);
  // off[0 .. n] = the exclusive scan of cap[k] = cnt[k * stride] (0 without
  // cnt) + key_ptr[k + 1] - key_ptr[k] (0 without key_ptr); off[n] = the total.
  int exclusive_scan(const uint64_t* key_ptr, const uint32_t* cnt, uint32_t stride, uint64_t n, uint64_t* off);
  void release();

 private:
  DevBuf caps_, part_;  // the n caps; the scan blocks' totals
};

}  // namespace ccrdt
