// Host side of a stage ("Host side of a stage"): what stands between an entry point's argument checks and its
// kernels.  DS_TRY ends a function at the first failing step, DS_LAUNCH launches and checks, allow_dynamic_lds lifts the
// 48 KiB limit of dynamic LDS, check_free refuses what does not fit, and Scratch holds the device memory of one call.
#pragma once

#include <memory>
#include <type_traits>

#include "ds_common.h"

#define DS_TRY(...)                                       \
    do {                                                  \
        const int ds_try_status_ = (__VA_ARGS__);         \
        if (ds_try_status_ != DS_OK) return ds_try_status_; \
    } while (0)

// A kernel name with a comma in its template arguments goes in parentheses, as for hipLaunchKernelGGL itself.
#define DS_LAUNCH(kernel, grid, block, lds, stream, ...)                                         \
    do {                                                                                         \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                       \
        hipError_t ds_launch_error_ = hipGetLastError();                                         \
        if (ds_launch_error_ != hipSuccess) return ::ds::hip_failed(ds_launch_error_, #kernel, __FILE__, __LINE__); \
    } while (0)

namespace ds {

// A kernel that asks for more than 48 KiB of dynamic LDS has to be allowed to, once, before its launch.
template <typename Kernel>
int allow_dynamic_lds(Kernel *kernel, size_t bytes)
{
    if (bytes > 48 * 1024)
        DS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(bytes)));
    return DS_OK;
}

// DS_E_HIP, with "<what>: needs <bytes> bytes of HBM, <free> are free", unless `bytes` and 64 MiB of head room for the
// kernels that follow are free on the current device (ds_runtime.hip).  `free_now` receives what was free.
int check_free(int64_t bytes, const char *what, size_t *free_now = nullptr);

// The device memory of one call, declared once: a stage names its pieces, allocate() checks that their sum fits,
// allocates them in the order of declaration (one hipMalloc each), uploads the staged ones, and the destructor frees
// them.  A piece of no elements stays a null pointer.  allocate() is called once, after the last declaration, and writes
// the slots: a body that shares a Scratch with its caller takes pointers to the caller's slots and reads them afterwards.
class Scratch {
public:
    template <typename T>
    void add(T **slot, size_t count)
    {
        pieces_.push_back({(void **)slot, count * sizeof(T), nullptr, nullptr});
    }
    template <typename T>
    void stage(T **slot, const typename std::remove_const<T>::type *host, size_t count)   // a piece that is filled from `host` (hipMemcpy, as upload())
    {
        pieces_.push_back({(void **)slot, count * sizeof(T), host, nullptr});
    }
    int64_t bytes() const
    {
        int64_t sum = 0;
        for (const Piece &piece : pieces_) sum += static_cast<int64_t>(piece.bytes);
        return sum;
    }
    int allocate(const char *what, int64_t also = 0)   // `also`: bytes the call allocates elsewhere, checked with the sum
    {
        if (allocated_) {
            set_error("%s: the scratch of a call is allocated once", what);
            return DS_E_ARG;
        }
        allocated_ = true;
        DS_TRY(check_free(bytes() + also, what));
        for (Piece &piece : pieces_) {
            if (piece.bytes) DS_HIP(hipMalloc(&piece.ptr, piece.bytes));
            *piece.slot = piece.ptr;
        }
        for (const Piece &piece : pieces_)
            if (piece.host && piece.bytes) DS_HIP(hipMemcpy(piece.ptr, piece.host, piece.bytes, hipMemcpyHostToDevice));
        return DS_OK;
    }
    ~Scratch()
    {
        for (const Piece &piece : pieces_)
            if (piece.ptr) (void)hipFree(piece.ptr);
    }
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;

private:
    struct Piece {
        void **slot;
        size_t bytes;
        const void *host;
        void *ptr;   // what the destructor frees: a slot may have gone out of scope by then
    };
    std::vector<Piece> pieces_;
    bool allocated_ = false;
};

}  // namespace ds
