// Host-side helpers shared by the engines behind include/cbdock.h: error reporting, tracked device allocations.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/cbdock.h"

// records the calling thread's last-error string (returned by cbd_last_error) and returns `code`
int cbd_fail(int code, const char* fmt, ...);
#define fail cbd_fail

#define HIPCHK(x)                                                                                              \
  do {                                                                                                         \
    hipError_t _e = (x);                                                                                       \
    if (_e != hipSuccess) return fail(CBD_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define CHK(x)            \
  do {                    \
    int _r = (x);         \
    if (_r != 0) return _r; \
  } while (0)

namespace cbd {

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

// The checkpoint tensors an engine was given (cbd_load_weight / cbd_conf_load_weight), by state_dict name
struct WeightStore {
  std::map<std::string, HostTensor> w;

  void load(const std::string& name, const float* data, const int64_t* shape, int32_t ndim) {
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(data, data + n);
    w[name] = std::move(t);
  }
  const HostTensor* find(const std::string& k) const {
    auto it = w.find(k);
    return it == w.end() ? nullptr : &it->second;
  }
  int need(const std::string& k, std::initializer_list<int64_t> shape, const HostTensor** out) const {
    const HostTensor* t = find(k);
    if (!t) return fail(CBD_ERR_WEIGHT, "missing tensor '%s' (load_state_dict strict=True)", k.c_str());
    if (t->shape != std::vector<int64_t>(shape)) return fail(CBD_ERR_WEIGHT, "tensor '%s' has an unexpected shape", k.c_str());
    *out = t;
    return 0;
  }
};

// Pairs of HIP events around the launches an engine times, and the running total of what they measured.  acquire() hands out the
// next pair (the caller records it); drain(lo, hi) reads pairs [lo, hi) into the total -- a pair whose time cannot be read (never
// recorded, e.g. a captured graph that was not replayed) is skipped.
struct EventPairPool {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs;
  size_t used = 0;

  hipError_t acquire(hipEvent_t* e0, hipEvent_t* e1) {
    if (used == pairs.size()) {
      hipEvent_t a, b;
      hipError_t r = hipEventCreate(&a);
      if (r == hipSuccess) r = hipEventCreate(&b);
      if (r != hipSuccess) return r;
      pairs.push_back({a, b});
    }
    *e0 = pairs[used].first; *e1 = pairs[used].second;
    ++used;
    return hipSuccess;
  }
  void destroy() {
    for (auto& p : pairs) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    pairs.clear();
    used = 0;
  }
};

struct KernelTimer {
  double total_ms = 0;
  int64_t n = 0;

  void drain(const EventPairPool& pool, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      float ms = 0.f;
      if (hipEventSynchronize(pool.pairs[i].second) == hipSuccess &&
          hipEventElapsedTime(&ms, pool.pairs[i].first, pool.pairs[i].second) == hipSuccess) {
        total_ms += ms;
        n += 1;
      }
    }
  }
  void report(double* avg_ms, int64_t* n_launches, double* total) const {
    if (avg_ms) *avg_ms = n ? total_ms / (double)n : 0.0;
    if (n_launches) *n_launches = n;
    if (total) *total = total_ms;
  }
  void reset() { total_ms = 0; n = 0; }
};

// CSR of an edge list [2][E] by its row 0 (the aggregating node), stable in the original column order: ptr [n_nodes + 1], and per
// slot the row-1 entry (dst) and the original column (eid).  The indices must have been range-checked.
inline void csr_by_row0(const int64_t* ei, int E, int n_nodes, std::vector<int>* ptr, std::vector<int>* dst, std::vector<int>* eid) {
  ptr->assign(n_nodes + 1, 0);
  for (int k = 0; k < E; ++k) (*ptr)[ei[k] + 1]++;
  for (int i = 0; i < n_nodes; ++i) (*ptr)[i + 1] += (*ptr)[i];
  dst->resize(E); eid->resize(E);
  std::vector<int> fillp(ptr->begin(), ptr->end() - 1);
  for (int k = 0; k < E; ++k) {
    const int p = fillp[ei[k]]++;
    (*dst)[p] = (int)ei[E + k];
    (*eid)[p] = k;
  }
}

// Device arena: bump allocation out of large hipMalloc'd chunks.  reset() rewinds without freeing, so the per-complex and
// per-batch workspaces of successive complexes re-use the same memory (a hipMalloc/hipFree pair per buffer costs more than
// the kernels of a small complex's set-up); release() returns everything to the runtime.
struct DevPool {
  struct Chunk { char* base; size_t size, used; };
  std::vector<Chunk> chunks;
  size_t cur = 0;
  hipStream_t stream = nullptr;   // uploads: nullptr = synchronous copies on the default stream; else asynchronous on this stream + wait (the host vector may go away)
  static constexpr size_t kChunk = size_t(64) << 20, kAlign = 256;

  hipError_t raw(void** out, size_t bytes) {
    bytes = (std::max<size_t>(bytes, 1) + kAlign - 1) / kAlign * kAlign;
    for (; cur < chunks.size(); ++cur) {
      Chunk& c = chunks[cur];
      if (c.size - c.used >= bytes) {
        *out = c.base + c.used;
        c.used += bytes;
        return hipSuccess;
      }
    }
    void* q = nullptr;
    const size_t sz = std::max(bytes, kChunk);
    hipError_t e = hipMalloc(&q, sz);
    if (e != hipSuccess) return e;
    chunks.push_back(Chunk{static_cast<char*>(q), sz, bytes});
    cur = chunks.size() - 1;
    *out = q;
    return hipSuccess;
  }
  template <typename T>
  hipError_t alloc(T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = raw(&q, n * sizeof(T));
    if (e == hipSuccess) *p = reinterpret_cast<T*>(q);
    return e;
  }
  template <typename T>
  hipError_t upload(T** p, const std::vector<T>& h) {
    hipError_t e = alloc(p, h.size());
    if (e != hipSuccess) return e;
    if (h.empty()) return e;
    if (!stream) return hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    e = hipMemcpyAsync(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
  }
  void reset() {
    for (Chunk& c : chunks) c.used = 0;
    cur = 0;
  }
  void release() {
    for (Chunk& c : chunks) (void)hipFree(c.base);
    chunks.clear();
    cur = 0;
  }
};

}  // namespace cbd
