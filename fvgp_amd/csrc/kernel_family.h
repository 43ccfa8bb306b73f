// The family of named stationary kernels, host side: what an ABI kernel id means, and the one place a launch picks its
// <KIND, D> instantiation.  The device side of the family is radial.h (radial<KIND>, radial_grad<KIND>, radial_hess<KIND>).
#pragma once
#include <type_traits>
#include "common.h"

// ABI id (enum fvgp_kernel_id, include/fvgp_hip.h) -> radial function (the KIND of radial.h: 0 rbf, 1 matern 3/2, 2 matern 5/2) and
// whether one length scale serves every dimension.  Every decoding of an id is a lookup here.
struct KernelFamilyEntry { int kind; bool iso; };
constexpr KernelFamilyEntry KERNEL_FAMILY[] = {
    {0, false},   // FVGP_KERNEL_RBF_ARD
    {1, false},   // FVGP_KERNEL_MATERN32_ARD
    {2, false},   // FVGP_KERNEL_MATERN52_ARD
    {0, true},    // FVGP_KERNEL_RBF_ISO
    {1, true},    // FVGP_KERNEL_MATERN32_ISO
    {2, true},    // FVGP_KERNEL_MATERN52_ISO
};
constexpr int KERNEL_FAMILY_COUNT = (int)(sizeof(KERNEL_FAMILY) / sizeof(KERNEL_FAMILY[0]));

inline bool kernel_id_known(int id) { return id >= 0 && id < KERNEL_FAMILY_COUNT; }

// hyperparameters the kernel owns: sigma^2, then one length scale or one per dimension (id: a known one)
inline int kernel_param_count(int id, int d) { return KERNEL_FAMILY[id].iso ? 2 : d + 1; }

// f(std::integral_constant<int, KIND>) for the radial function `kind` (a KERNEL_FAMILY kind)
template <class F>
inline void dispatch_kind(int kind, F &&f) {
    switch (kind) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        default: f(std::integral_constant<int, 2>{}); break;
    }
}

// f(KIND, D) with the dimensions that have an instantiation of their own; D = 0 is the runtime dimension (<= FVGP_MAX_DIM)
template <class F>
inline void dispatch_kind_dim(int kind, int d, F &&f) {
    dispatch_kind(kind, [&](auto KIND) {
        switch (d) {
            case 1: f(KIND, std::integral_constant<int, 1>{}); break;
            case 2: f(KIND, std::integral_constant<int, 2>{}); break;
            case 3: f(KIND, std::integral_constant<int, 3>{}); break;
            case 4: f(KIND, std::integral_constant<int, 4>{}); break;
            default: f(KIND, std::integral_constant<int, 0>{}); break;
        }
    });
}
