// c_boundary.hpp -- the guards of the C boundary that the codec's and the RGB-D source's entry points share: where the log's errors
// go while an entry runs, and what becomes of a C++ exception in its body.
#pragma once

#include "internal.hpp"

#include <exception>

namespace cwipc_amd {

// The caller's errorMessage is where the log's errors go for as long as an entry point runs.
struct ErrorbufScope {
    explicit ErrorbufScope(char **errorMessage) { cwipc_log_set_errorbuf(errorMessage); }
    ~ErrorbufScope() { cwipc_log_set_errorbuf(nullptr); }
};

// No exception crosses the C boundary: what the standard library throws in a call's body (memory) is logged and becomes its error value.
template <typename T, typename Body>
T guarded(const char *who, T failed, Body &&body) {
    try {
        return body();
    } catch (const std::exception &e) {
        note_error(who, e.what());
    } catch (...) {
        note_error(who, "unknown exception");
    }
    return failed;
}

}  // namespace cwipc_amd
