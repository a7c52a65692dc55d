// Ownership of device memory by type.  DevBuf<T> owns one device allocation, Ref<T> shares one reference-counted host object.
// No HIP include: the device is reached through the two functions declared first, which the library defines (pa_capi.hip) and a
// host-only check replaces by counting stand-ins (tests/cpu/devbuf_check.cpp).
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace pa {

void *dev_malloc_bytes(size_t bytes);    // never nullptr: throws pa::Error
void dev_free_bytes(void *p) noexcept;   // p != nullptr

// buffers a DevBuf owns at this moment, process-wide (pa_device_buffers_live)
inline std::atomic<int64_t> g_dev_buffers_live{0};

template <typename T>
class DevBuf;
template <typename T>
DevBuf<T> dev_alloc(size_t n);

// Move-only owner of a device array: one pointer, freed by the destructor and by reset().  Reads as the T * it holds wherever an
// lvalue stands (kernel arguments, null tests, pointer arithmetic); a temporary does not convert, so the result of dev_alloc /
// dev_upload has to be given an owner.
template <typename T>
class DevBuf {
public:
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, o.p_ = nullptr;
    }
    return *this;
  }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { reset(); }

  void reset() noexcept {
    if (!p_) return;
    dev_free_bytes(p_);
    --g_dev_buffers_live;
    p_ = nullptr;
  }
  T *get() const { return p_; }
  // hands the array to the caller, who frees it with hipFree (it leaves the live count)
  T *release() noexcept {
    T *p = p_;
    if (p) --g_dev_buffers_live;
    p_ = nullptr;
    return p;
  }
  operator T *() const & { return p_; }
  operator T *() && = delete;

private:
  friend DevBuf dev_alloc<T>(size_t n);
  explicit DevBuf(T *p) : p_(p) {}
  T *p_ = nullptr;
};

template <typename T>
DevBuf<T> dev_alloc(size_t n) {
  T *p = static_cast<T *>(dev_malloc_bytes((n ? n : 1) * sizeof(T)));
  ++g_dev_buffers_live;
  return DevBuf<T>(p);
}

// Shared ownership of a host object that carries its own count (T::refcount): a copy adds a reference, the destructor drops one
// and deletes the object at zero.  Ref(p) adds a reference to whatever count p already has, so an object whose creator keeps
// a reference without a handle (pa_geom: the caller's, dropped by pa_geom_destroy) starts at 1 and any other at 0.
template <typename T>
class Ref {
public:
  Ref() = default;
  explicit Ref(T *p) : p_(p) {
    if (p_) ++p_->refcount;
  }
  Ref(const Ref &o) : Ref(o.p_) {}
  Ref(Ref &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  Ref &operator=(Ref o) noexcept {
    std::swap(p_, o.p_);
    return *this;
  }
  ~Ref() { drop(p_); }
  // one reference less, by whoever held it
  static void drop(T *p) {
    if (p && --p->refcount == 0) delete p;
  }
  T *get() const { return p_; }
  T *operator->() const { return p_; }
  T &operator*() const { return *p_; }
  operator T *() const { return p_; }

private:
  T *p_ = nullptr;
};

}  // namespace pa
