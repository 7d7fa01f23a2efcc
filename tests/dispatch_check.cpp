// stand-alone host check of dpx_device.hpp's dispatchers: which (C / R, parity, flag) reaches the callable, and the error for values off the list
#include <cstdio>
#include <vector>
#include "dpx_device.hpp"
using namespace dpx_dev;
int main() {
    int bad = 0;
    for (int v = -2; v <= 20; v++) {
        int got = -1;
        hipError_t e = dispatch_int<2, 4, 8, 16>(v, [&](auto r) { got = decltype(r)::value; return hipSuccess; });
        const bool on = v == 2 || v == 4 || v == 8 || v == 16;
        if (on ? (e != hipSuccess || got != v) : (e != hipErrorInvalidValue || got != -1)) { bad++; std::printf("dispatch_int %d -> %d err %d\n", v, got, (int)e); }
    }
    hipError_t passed = dispatch_int<8>(8, [&](auto) { return hipErrorOutOfMemory; });
    if (passed != hipErrorOutOfMemory) { bad++; std::printf("error of the callable lost\n"); }
    for (int C = 0; C <= 9; C++) for (int band = 1; band <= 4; band++) for (int flag = 0; flag < 2; flag++) {
        int c = -1, pb = -1, f = -1, calls = 0;
        hipError_t e = dispatch_fill(C, band, flag != 0, [&](auto cc, auto pp, auto ff) { c = decltype(cc)::value; pb = decltype(pp)::value; f = decltype(ff)::value; calls++; return hipSuccess; });
        const bool on = C == 1 || C == 2 || C == 4 || C == 8;
        const int wantPb = ((band + 1) & 1) != 0;
        if (on ? (e != hipSuccess || c != C || pb != wantPb || f != flag || calls != 1) : (e != hipErrorInvalidValue || calls != 0)) { bad++; std::printf("dispatch_fill C=%d band=%d flag=%d -> %d %d %d calls %d err %d\n", C, band, flag, c, pb, f, calls, (int)e); }
    }
    std::printf(bad ? "FAILED %d\n" : "dispatchers ok\n", bad);
    return bad != 0;
}
