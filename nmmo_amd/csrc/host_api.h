// host_api.h — what the C interface of every library (capi.hip, heads.hip, ppo.hip, lstm.hip)
// shares. Host code only: the per-thread error text behind <prefix>_last_error() and the string
// <prefix>_build_info() returns. Each library keeps its own copy (internal linkage) and exports
// the two functions under its own names.
#pragma once

#include <stdarg.h>
#include <stdio.h>

#include <string>

// build.py passes the library's source hash (build.source_hash(name)) to every translation unit
#ifndef NMMO_SRC_HASH
#define NMMO_SRC_HASH "unknown"
#endif
#define NMMO_BUILD_INFO "src=" NMMO_SRC_HASH " arch=gfx950 fp_contract=off"

namespace {

thread_local std::string g_err;

// records the message for <prefix>_last_error() and returns `code`: `return fail(E, "...", ...)`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

}  // namespace
