// partial_sums.h — the one stage through which the BAL front end reads per-workgroup partial sums back (design/25_partial_sums.md): a
// kernel's last thread writes partials[blockIdx.x]; the sets of one host round trip lie packed in one device buffer, are copied to
// pinned memory once, and are added on the host in index order.
#ifndef CERES_HIP_PARTIAL_SUMS_H_
#define CERES_HIP_PARTIAL_SUMS_H_

#include <algorithm>
#include <string>

namespace chip {

struct PartialSet { int offset = 0, count = 0; };

// The bookkeeping alone, no HIP in it (tests/test_partial_sums_cpu.py compiles it with g++).  Sets carry no generation: a set is good
// from its take() to the first room() after the collect() or drop() that follows — holding one longer is the caller's mistake.
struct PartialLedger {
  int capacity = 0;
  int position = 0;   // doubles taken since the last collect() / drop()
  int granted = 0;    // end of what the last room() granted: take() stays below it
  std::string error;  // why the last room() or take() was refused; kept until reported
  // the offset at which `max_doubles` more fit; -1 (and nothing changes): they do not
  int room(int max_doubles) {
    if (max_doubles < 0 || max_doubles > capacity - position) {
      error = "partial sums: room for " + std::to_string(max_doubles) + " doubles asked, " + std::to_string(capacity - position) + " of " +
              std::to_string(capacity) + " free";
      return -1;
    }
    granted = position + max_doubles;
    return position;
  }
  // the next `count` doubles — what the kernel just launched wrote from room()'s offset on; more than room() granted: an empty set
  PartialSet take(int count) {
    if (count < 0 || count > granted - position) {
      error = "partial sums: " + std::to_string(count) + " doubles taken, " + std::to_string(granted - position) + " granted";
      return PartialSet{position, 0};
    }
    position += count;
    return PartialSet{position - count, count};
  }
  void drop() { position = granted = 0; }   // sums nobody reads
  // the refusal's message, once: the caller abandons its round trip
  std::string refusal() { std::string why; why.swap(error); drop(); return why; }
};

#ifdef __HIPCC__
struct PartialSums : PartialLedger {
  double *device = nullptr, *pinned = nullptr;   // `capacity` doubles each (pinned: hipHostMalloc)
  double* room(int max_doubles) { const int at = PartialLedger::room(max_doubles); return at < 0 ? nullptr : device + at; }
  // ONE copy of [0, position), ONE synchronisation; the sets handed out stay readable until the next room()
  hipError_t collect(hipStream_t stream) {
    const hipError_t e = position > 0 ? hipMemcpyAsync(pinned, device, sizeof(double) * position, hipMemcpyDeviceToHost, stream) : hipSuccess;
    drop();
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
  }
  double* host(PartialSet set) const { return pinned + set.offset; }
  double sum(PartialSet set) const {   // on the pinned copy, in index order from 0: deterministic
    double v = 0;
    for (int i = 0; i < set.count; ++i) v += pinned[set.offset + i];
    return v;
  }
  double max(PartialSet set) const {
    double v = 0;
    for (int i = 0; i < set.count; ++i) v = std::max(v, pinned[set.offset + i]);
    return v;
  }
};
#endif  // __HIPCC__

}  // namespace chip
#endif  // CERES_HIP_PARTIAL_SUMS_H_
