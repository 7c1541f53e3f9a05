// gte_own.h — the owner of ONE block of memory that its holder may replace, and the rules by which such a block
// grows.  Nothing of HIP or of csrc/ is included: tests/own_check.cpp drives it with malloc / free; gte_host.h binds
// it to hipFree and hipHostFree.  The owner waits for nothing: whoever lets a block go has waited for its users.
#pragma once

#include <cstddef>

namespace gte_own {

// The size a block gets when `need` bytes (or entries) are asked of one that has `have`: exactly that; half as
// much again; or at least double (max(need, 2 * have)), a block that is large enough staying as it is.
inline size_t grow_exact(size_t, size_t need) { return need; }
inline size_t grow_by_half(size_t, size_t need) { return need + need / 2; }
inline size_t grow_doubling(size_t have, size_t need) { return have >= need ? have : need > 2 * have ? need : 2 * have; }

// One block: a pointer, its byte count and Release, which is called exactly once per block adopted.  Move-only.
template <void (*Release)(void*)>
class Block {
 public:
  Block() = default;
  Block(Block&& o) noexcept { *this = static_cast<Block&&>(o); }
  Block& operator=(Block&& o) noexcept {
    if (this != &o) {
      replace(o.ptr_, o.bytes_);
      o.ptr_ = nullptr;
      o.bytes_ = 0;
    }
    return *this;
  }
  ~Block() { reset(); }
  // the old block is released, `fresh` (allocated by the caller: allocate, THEN free the old) adopted
  void replace(void* fresh, size_t bytes) {
    reset();
    ptr_ = fresh;
    bytes_ = bytes;
  }
  // release now; nothing happens to an empty owner
  void reset() {
    if (ptr_) Release(ptr_);
    ptr_ = nullptr;
    bytes_ = 0;
  }
  void* get() const { return ptr_; }
  template <typename T> T* as() const { return static_cast<T*>(ptr_); }
  size_t bytes() const { return bytes_; }

 private:
  void* ptr_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace gte_own
