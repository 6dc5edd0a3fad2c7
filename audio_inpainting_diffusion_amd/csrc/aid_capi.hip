// ABI version + last-error plumbing of libaid_hip.so, and the device zero page.
#include <string.h>
#include "aid_common.h"

static char g_last_error[256] = "";

void aid_set_error(const char* msg) {
    strncpy(g_last_error, msg ? msg : "", sizeof(g_last_error) - 1);
    g_last_error[sizeof(g_last_error) - 1] = 0;
}

// Name of the device kernel the most recent aid_conv2d call dispatched to (measurement aid: bench.py groups conv launch
// times per kernel family with it).  Host-side bookkeeping only.
static const char* g_last_kernel = "";
void aid_note_kernel(const char* name) { g_last_kernel = name ? name : ""; }
extern "C" const char* aid_last_kernel(void) { return g_last_kernel; }

// 256 bytes of zeros in device memory: what the direct-to-LDS kernels read where a piece lies outside the tensor.  Device symbols are per translation
// unit without -fgpu-rdc, so the kernels cannot name this one: every launcher passes the pointer by value.  Looked up once.
__device__ float4 g_aid_zero_page[16];
const float* aid_zero_page() {
    static const float* zero = nullptr;
    if (!zero) {
        void* z = nullptr;
        if (hipGetSymbolAddress(&z, HIP_SYMBOL(g_aid_zero_page)) != hipSuccess) { aid_set_error("aid_conv2d: zero page lookup failed"); return nullptr; }
        zero = (const float*)z;
    }
    return zero;
}

extern "C" int aid_abi_version(void) { return AID_ABI_VERSION; }
extern "C" const char* aid_last_error(void) { return g_last_error; }
