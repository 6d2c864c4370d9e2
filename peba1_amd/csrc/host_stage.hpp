// host_stage.hpp -- the engine's one pinned host staging area (host side, no device code).
//
// A call that returns without a host wait must not leave the GPU reading host memory the caller may release or
// overwrite: the small lists such a call uploads (slot lists, index lists, descriptors) are copied here first.  The area
// bump-allocates, and one event stands behind the calls that uploaded from it.  Where a reservation goes is stage_place,
// a pure function that tests/test_host_stage_cpu.py drives through tfhe_hip_test_stage_place on a machine without a GPU.
// Not a file the kernels are built from (peba1_amd/kernel_id.py).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>

namespace tfhe_hip {

constexpr size_t STAGE_ALIGN = 16, STAGE_START_BYTES = (size_t)256 << 10;

// offset: where the reservation lies; wait: the event is waited for first -- not the stream -- and everything reserved
// before is then free; capacity: what the area holds afterwards (reallocated where that differs); next: the write position
struct StagePlace { size_t offset; bool wait; size_t capacity, next; };
inline StagePlace stage_place(size_t pos, size_t capacity, bool outstanding, size_t bytes) {
    const auto up = [](size_t v) { return (v + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1); };
    const size_t at = up(pos), need = up(bytes);
    if (at + need <= capacity) return {at, false, capacity, at + need};
    // from offset 0 again, behind the uploads that still read the area; growth is by half again beyond the request
    return {0, outstanding, need > capacity ? std::max(STAGE_START_BYTES, up(need + need / 2)) : capacity, need};
}

// Owned by the engine and used under the recorder lock like the rest of it (bodies in engine.cpp).  A call fills what it
// reserved and enqueues the uploads that read it; it ends in a synchronised stream (idle) or in uploaded().  A later
// reservation may start from offset 0: the wait in front of it keeps it off every list that is still to be read.
class Engine;
class HostStage {
public:
    explicit HostStage(Engine &owner) : owner_(owner) {}
    void *reserve(size_t bytes);         // 16-byte aligned pinned memory, valid until the device has read the uploads from it
    void uploaded();                     // those uploads are enqueued: records the area's event on the engine's stream
    void wait();                         // for that event, bounded like every host wait (recorded now if it was not)
    void idle() { outstanding_ = false; }   // the engine's stream was synchronised: nothing reads the area any more
private:
    Engine &owner_;
    char *base_ = nullptr;
    size_t capacity_ = 0, pos_ = 0;
    hipEvent_t event_ = nullptr;
    bool outstanding_ = false, recorded_ = false;       // reserved since the last wait or idle / the event stands behind it
};

}  // namespace tfhe_hip
