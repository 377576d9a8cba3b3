// capi_error.h -- the error report of the C ABI, shared by the entry points of all three public headers.
#pragma once

namespace sigma {

// Formats the calling thread's error text -- what sigma_scan_last_error() returns -- and hands `code` back, so that a
// refusal reads `return fail(code, "...", values);`.  Defined in capi.hip.  Nothing calls it on a success path.
// Internal to the library: not part of include/.
__attribute__((visibility("hidden"), format(printf, 2, 3))) int fail(int code, const char* fmt, ...);

}  // namespace sigma
