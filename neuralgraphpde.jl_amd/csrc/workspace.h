// workspace.h -- how every entry with a caller-provided workspace sizes it and carves it.  A site writes ONE function that takes its
// pieces from a Workspace& in order and fills the struct of pointers its entry uses; the *_workspace_bytes query runs that function
// on a measuring Workspace (no base) and reads bytes(), the entry runs it on the caller's buffer after check_workspace.  The size
// and the offsets cannot drift apart: they are the same arithmetic.  Plain C++, no HIP include: it compiles with a host compiler alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/ngpde.h"

namespace ngpde {

int32_t fail(int32_t code, const char *fmt, ...);   // (common.h) records the message, returns the code

constexpr size_t kGranule = 256;   // every piece starts on a multiple of this from the base
inline size_t round_up256(size_t bytes) { return (bytes + (kGranule - 1)) & ~(kGranule - 1); }
constexpr size_t kWsSlack = 256;   // what the Dense, GAT and message-MLP workspace queries add behind their pieces

// A bump allocator over bytes in 256-byte granules.  Without a base it only measures: take() returns nullptr and advances.
class Workspace {
 public:
  explicit Workspace(void *base = nullptr) : base_(static_cast<char *>(base)) {}
  template <class T>
  T *take(size_t count) {
    char *p = base_ ? base_ + at_ : nullptr;
    at_ += round_up256(count * sizeof(T));
    return reinterpret_cast<T *>(p);
  }
  size_t bytes() const { return at_; }   // what has been taken so far = the offset of the next piece

 private:
  char *base_;
  size_t at_ = 0;
};

// the bytes of a layout function called as layout(Workspace &, args...)
template <class Layout, class... Args>
size_t measure(Layout layout, Args &&...args) {
  Workspace w;
  layout(w, args...);
  return w.bytes();
}

// The only place that raises NGPDE_ERR_WORKSPACE.  align: the power of two the base must be a multiple of; 1: not tested
inline int32_t check_workspace(const char *fn, const void *workspace, size_t workspace_bytes, size_t needed, int align) {
  if (!workspace || workspace_bytes < needed)
    return fail(NGPDE_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, needed);
  if (reinterpret_cast<uintptr_t>(workspace) & (uintptr_t)(align - 1))
    return fail(NGPDE_ERR_INVALID_ARGUMENT, "%s: the workspace is not %d-byte aligned", fn, align);
  return NGPDE_OK;
}

}  // namespace ngpde
