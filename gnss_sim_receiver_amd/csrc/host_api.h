// host_api.h — the host helpers gnsship_abi.hip defines for every translation unit of the C-ABI layer.
#pragma once
#include "engine.h"

namespace gnsship {
int fail(gnsship_ctx* ctx, int code, const char* what);           // last_error = what (copied); returns code
int hip_fail(gnsship_ctx* ctx, hipError_t e, const char* where);  // last_error = "where: <HIP's text>"; E_NOMEM or E_DEVICE
int set_device(gnsship_ctx* ctx);
}  // namespace gnsship
