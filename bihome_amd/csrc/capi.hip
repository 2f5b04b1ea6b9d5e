// Library probe entry points.
#include "common.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>


thread_local BhQuery* bh_query_ctx = nullptr;


bool bh_query(const char* fmt, ...) {
    BhQuery* q = bh_query_ctx;
    if (!q) return false;
    if (q->len && q->len < (int)sizeof(q->name) - 1) q->name[q->len++] = '+';
    va_list ap;
    va_start(ap, fmt);
    const int room = (int)sizeof(q->name) - q->len;
    const int w = vsnprintf(q->name + q->len, (size_t)room, fmt, ap);
    va_end(ap);
    if (w > 0) q->len += w < room ? w : room - 1;
    return true;
}

extern "C" {

int bh_version(void) { return 2; }


int bh_device_arch(char* buf, int buflen) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, 0);
    if (e != hipSuccess) return (int)e;
    if (buf && buflen > 0) {
        strncpy(buf, prop.gcnArchName, (size_t)buflen - 1);
        buf[buflen - 1] = 0;
    }
    return BH_OK;
}

int bh_conv_variant(const bh_conv_desc* d, int which, int accumulate, int with_bnstats /* = bn_groups */, char* buf, int n) {
    if (!d || !buf || n < 2 || which < 0 || which > 6) return BH_E_BADARG;
    BhQuery q;
    q.name[0] = 0; q.len = 0;
    // non-null placeholders: in query mode no kernel is launched and no pointer is dereferenced
    float* p = reinterpret_cast<float*>(static_cast<uintptr_t>(256));
    double* pd = reinterpret_cast<double*>(static_cast<uintptr_t>(256));
    bh_query_ctx = &q;
    int rc;
    if (which == 0) rc = with_bnstats ? bh_conv_fwd_bnstats(p, p, nullptr, p, d, pd, with_bnstats, nullptr) : bh_conv_fwd(p, p, nullptr, p, d, nullptr);
    else if (which == 1) rc = bh_conv_dgrad(p, p, p, d, accumulate, nullptr);
    else if (which == 2) rc = bh_conv_wgrad(p, p, p, nullptr, d, nullptr);
    else if (which == 3) rc = bh_conv_wgrad_det(p, p, p, nullptr, d, p, 1ll << 40, nullptr);      // 3: the workspace form
    else if (which == 6) rc = bh_conv_dgrad_colsum(p, p, p, d, pd, nullptr);
    else {                                                                        // 4 / 5: bh_conv_dgrad_bnreduce, mask from z / from y
        bh_bn_reduce bnr = {};
        bnr.z = p; bnr.y = which == 5 ? p : nullptr; bnr.stats = pd; bnr.gamma = p; bnr.beta = p; bnr.eps = 1e-5f; bnr.relu = 1;
        rc = bh_conv_dgrad_bnreduce(p, p, p, d, accumulate, &bnr, pd, with_bnstats > 0 ? with_bnstats : 1, nullptr);
    }
    bh_query_ctx = nullptr;
    if (rc) return rc;
    strncpy(buf, q.name, (size_t)n - 1);
    buf[n - 1] = 0;
    return BH_OK;
}

}  // extern "C"
