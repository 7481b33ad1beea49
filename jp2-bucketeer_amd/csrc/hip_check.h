// hip_check.h -- HIPCHECK(call): on a HIP error, sets the enclosing function's
// `std::string err` to the call's text and the error string, and returns false.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#define HIPCHECK(x)                                                                    \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            err = std::string(#x) + ": " + hipGetErrorString(e_);                      \
            return false;                                                              \
        }                                                                              \
    } while (0)
