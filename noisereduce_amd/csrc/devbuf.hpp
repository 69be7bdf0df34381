// A device allocation its holder owns: freed with the holder (the handle, a stream bank, a clips or rows session).  Whoever
// deletes the holder has synchronised what may still read the buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace sg {
namespace host {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // the other buffer's allocation; this one's goes
  void take(DevBuf& o) {
    release();
    p = o.p;
    bytes = o.bytes;
    o.p = nullptr;
    o.bytes = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

}  // namespace host
}  // namespace sg
