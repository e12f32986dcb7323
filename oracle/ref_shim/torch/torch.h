// ORACLE — test infrastructure only.  The few at:: names the host wrappers of the reference's operator files mention, so that those files compile without torch
// headers or libtorch: a Tensor is a device pointer, every tensor is float / contiguous / on the device (the drivers under oracle/ guarantee it), and the floating
// dispatch runs its body once with scalar_t = float (the reference's Python casts to float before every call).
#pragma once
#include <optional>
#include <stdint.h>

namespace at {
enum class ScalarType { Byte, Int, Half, Float, Double };
struct Device {
    bool is_cuda() const { return true; }
};
struct Tensor {
    void* ptr = nullptr;
    Tensor() = default;
    explicit Tensor(const void* p) : ptr(const_cast<void*>(p)) {}
    template <typename T> T* data_ptr() const { return static_cast<T*>(ptr); }
    ScalarType scalar_type() const { return ScalarType::Float; }
    Device device() const { return Device(); }
    bool is_contiguous() const { return true; }
};
template <typename T> using optional = std::optional<T>;
}  // namespace at

#define TORCH_CHECK(cond, ...) ((void)(cond))
#define AT_DISPATCH_FLOATING_TYPES_AND_HALF(TYPE, NAME, ...) \
    do {                                                      \
        (void)(TYPE);                                         \
        using scalar_t = float;                               \
        (__VA_ARGS__)();                                      \
    } while (0)
