// bx_loader_stubs.cpp -- link-time stand-in for the one symbol csrc/hostio.cpp takes from the rest of the library, for
// tests/c/bx_loader_san.cpp only: the loader is linked alone, without the device runtime.  The last error text is kept so that the
// program can print it.
#include <cstdarg>
#include <cstdio>

namespace qa {
char g_last_error[1024] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
}
}  // namespace qa
