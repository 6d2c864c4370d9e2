// device_buf.hpp -- the owner of device memory whose exhaustion is recoverable (engine.cpp "recoverable_alloc").  Host only.
#pragma once
#include <cstddef>
#include <utility>

namespace tfhe_hip {

// engine.cpp: hipMalloc under the library's accounting and the test cap -- a full card is an ApiError that names `what`,
// with nothing changed -- and hipFree of what it returned, with the same byte count (a null pointer: nothing)
void *recoverable_alloc(size_t bytes, const char *what);
void recoverable_free(void *p, size_t bytes);

// `count` elements of T from ONE recoverable_alloc, given back by reset() or the destructor; move-only.  An ApiError that
// unwinds through a run of these gives back what was allocated so far: "the call had no effect, nothing is held".
template <class T>
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(size_t count, const char *what) : p_(static_cast<T *>(recoverable_alloc(count * sizeof(T), what))), bytes_(count * sizeof(T)) {}
    DeviceBuf(DeviceBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DeviceBuf &operator=(DeviceBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    ~DeviceBuf() { reset(); }
    void reset() { recoverable_free(std::exchange(p_, nullptr), std::exchange(bytes_, 0)); }
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
    bool empty() const { return !p_; }
private:
    T *p_ = nullptr;
    size_t bytes_ = 0;
};

}  // namespace tfhe_hip
