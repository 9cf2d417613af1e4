// common_host.hpp — error plumbing for the C ABI (int status + thread-local message).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/ragmi.h"

namespace ragmi {

inline std::string& last_error() {
  static thread_local std::string msg;
  return msg;
}

inline void clear_error() { last_error().clear(); }

inline int fail(int code, const std::string& msg) {
  last_error() = msg;
  return code;
}

// ---- diagnostic A/B knobs -------------------------------------------
// The RAGMI_* environment variables that switch kernels for A/B measurements (scan grid,
// seed sample, rescan grid, GEMM variant, LayerNorm modes, ...) are honoured only while a
// handle of this process created with RAG_CREATE_DIAGNOSTIC (rag_index_create_ex's storage
// argument, rag_encoder_create_ex's flags) is alive: a successful create counts it, its
// destroy releases it, and the first one says so on stderr. Otherwise every knob reads as its
// production default, and a knob that is set but ignored is reported once on stderr, so a
// stray variable in a serving process cannot change results or speed unnoticed.
inline std::atomic<int>& diagnostic_handles() {
  static std::atomic<int> n{0};
  return n;
}
inline void diagnostic_acquire() {
  static std::atomic<bool> said{false};
  diagnostic_handles().fetch_add(1);
  if (!said.exchange(true))
    std::fprintf(stderr, "ragmi: diagnostic handle created: RAGMI_* A/B knobs are honoured "
                         "while diagnostic handles live\n");
}
inline void diagnostic_release() { diagnostic_handles().fetch_sub(1); }

class Knob {
 public:
  explicit Knob(const char* name) : name_(name) {
    const char* v = std::getenv(name);
    set_ = v != nullptr;
    if (set_) text_ = v;
  }
  // integer value when honoured, else `dflt`
  int get(int dflt) {
    if (!honoured()) return dflt;
    return std::atoi(text_.c_str());
  }
  // string value when honoured, else nullptr
  const char* str() { return honoured() ? text_.c_str() : nullptr; }

 private:
  bool honoured() {
    if (!set_) return false;
    if (diagnostic_handles().load(std::memory_order_relaxed) > 0) return true;
    if (!warned_.exchange(true))
      std::fprintf(stderr,
                   "ragmi: %s=%s ignored: A/B knobs need a handle created with "
                   "RAG_CREATE_DIAGNOSTIC\n",
                   name_, text_.c_str());
    return false;
  }
  const char* name_;
  bool set_ = false;
  std::string text_;
  std::atomic<bool> warned_{false};
};

// ---- device buffers of the host layers (index_*.hip, bert_capi.hip) ----------------------
// a hipMalloc buffer freed on every return path; release() hands it to a longer-lived owner
template <typename T>
struct DeviceBuf {
  T* p = nullptr;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  ~DeviceBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  T* release() {
    T* r = p;
    p = nullptr;
    return r;
  }
};

// One device buffer of a workspace: where its pointer lives, its size (0: not part of this
// configuration), zeroed at creation or not. A group of buffers that live and grow together
// is a table of these (a std::array returned by one function), in allocation order.
struct WsBuf {
  void** p;
  size_t bytes;
  bool zero;
};
template <typename T>
WsBuf ws_buf(T*& p, size_t bytes, bool zero = false) {
  return {reinterpret_cast<void**>(&p), bytes, zero};
}

// frees what the table's buffers hold and nulls them
template <typename Bufs>
void ws_free_all(const Bufs& bufs) {
  for (const WsBuf& b : bufs) {
    if (*b.p) (void)hipFree(*b.p);
    *b.p = nullptr;
  }
}

// One hipMalloc per buffer, in the table's order (the buffers hold nothing before), then the
// memsets. All or none: a failure frees what was allocated, so a group is never half-filled.
template <typename Bufs>
hipError_t ws_alloc_all(const Bufs& bufs) {
  hipError_t e = hipSuccess;
  for (const WsBuf& b : bufs)
    if (b.bytes && e == hipSuccess && (e = hipMalloc(b.p, b.bytes)) != hipSuccess) *b.p = nullptr;
  for (const WsBuf& b : bufs)
    if (b.zero && e == hipSuccess) e = hipMemset(*b.p, 0, b.bytes);
  if (e != hipSuccess) ws_free_all(bufs);
  return e;
}

}  // namespace ragmi

#define RAG_HIP(expr)                                                                  \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return ragmi::fail(_e == hipErrorOutOfMemory ? RAG_ENOMEM : RAG_EHIP,             \
                         std::string(#expr) + ": " + hipGetErrorString(_e));            \
  } while (0)
