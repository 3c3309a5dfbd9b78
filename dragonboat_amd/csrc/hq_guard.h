// hq_guard.h — the one exception guard of the C entries of the step worker (hq_worker*.cpp,
// hq_jobs.cpp), the wire (hq_wire.cpp) and the event stream (hq_stream*.cpp, hq_task_pool.h): no
// C++ exception crosses the C-ABI. An entry's body runs inside hq::guard; what
// it returns is the entry's code, what it throws becomes one:
//   std::bad_alloc, std::length_error   HQ_E_NOMEM  "<entry>: out of memory"
//   std::system_error                   HQ_E_NOMEM  "<entry>: <what()>"
//   anything else                       HQ_E_STATE  "<entry>: unexpected exception"
// `record(code, message)` keeps the message where the entry's caller reads it (a worker's
// hq_worker_last_error, a wire's hq_wire_last_error); an entry without a handle has nowhere to
// keep one and uses the form without `record`: the code alone. Nothing but the standard library
// and the error codes.
#pragma once
#include <new>
#include <stdexcept>
#include <string>
#include <system_error>

#include "../../include/hipquorum.h"

namespace hq {

// (recording allocates the message: when that fails too, the code alone is returned)
template <class Record>
int guard_report(const char *entry, const char *text, int code, Record &record) noexcept {
    try {
        record(code, std::string(entry) + ": " + text);
    } catch (...) {
    }
    return code;
}

template <class Record, class Body>
int guard(const char *entry, Record &&record, Body &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return guard_report(entry, "out of memory", HQ_E_NOMEM, record);
    } catch (const std::length_error &) {
        return guard_report(entry, "out of memory", HQ_E_NOMEM, record);
    } catch (const std::system_error &e) {
        return guard_report(entry, e.what(), HQ_E_NOMEM, record);
    } catch (...) {
        return guard_report(entry, "unexpected exception", HQ_E_STATE, record);
    }
}

template <class Body>
int guard(const char *entry, Body &&body) noexcept {
    return guard(entry, [](int, const std::string &) {}, body);
}

}  // namespace hq
