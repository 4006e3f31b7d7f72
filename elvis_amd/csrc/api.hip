// ABI version, thread-local error string and last-launched kernel name for the C boundary.
#include "common.h"
#include <string.h>

static thread_local char g_err[512] = "";
static thread_local const char* g_last_launch = "";

void elvis_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

void elvis_note_launch(const char* name) { g_last_launch = name; }

extern "C" int elvis_abi_version(void) { return ELVIS_ABI_VERSION; }
extern "C" const char* elvis_last_error(void) { return g_err; }
extern "C" const char* elvis_last_launch(void) { return g_last_launch; }
