// Host-only harness around gauss_newton.h's plain C++ part (solve_damped, rot_exp), built with g++ by
// tests/test_gauss_newton_cpu.py: no HIP header.  Reads one query per line of standard input, every number a hex float, and prints one
// line per query, every number a hex float:
//   solve LD n damping tot[0 .. LD (LD + 1) / 2 + LD)   ->  "refused" or the n values of the solution      (LD 7 or 8)
//   rot w0 w1 w2                                        ->  Rx (9, row-major), V (9), and Rx again as computed without V (9)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../coivo_amd/csrc/gauss_newton.h"
using namespace colvo;

template <int LD>
static void solve(char* p) {
    const int n = (int)strtol(p, &p, 10);
    const double damping = strtod(p, &p);
    double tot[LD * (LD + 1) / 2 + LD], A[LD][LD], xs[LD];
    for (double& v : tot) v = strtod(p, &p);
    if (n < 1 || n > LD || !gn::solve_damped<LD>(A, xs, tot, n, damping)) {
        puts(n < 1 || n > LD ? "bad n" : "refused");
        return;
    }
    for (int k = 0; k < n; ++k) printf("%a%c", xs[k], k + 1 < n ? ' ' : '\n');
}

int main() {
    static char line[8192];
    while (fgets(line, sizeof line, stdin)) {
        char* p = line;
        if (!strncmp(p, "solve ", 6)) {
            const int LD = (int)strtol(p + 6, &p, 10);
            if (LD == 8) solve<8>(p);
            else if (LD == 7) solve<7>(p);
            else puts("bad LD");
        } else if (!strncmp(p, "rot ", 4)) {
            p += 4;
            const double w0 = strtod(p, &p), w1 = strtod(p, &p), w2 = strtod(p, &p);
            double Rx[3][3], V[3][3], R1[3][3];
            gn::rot_exp(w0, w1, w2, Rx, V);
            gn::rot_exp(w0, w1, w2, R1, nullptr);
            for (int k = 0; k < 9; ++k) printf("%a ", Rx[k / 3][k % 3]);
            for (int k = 0; k < 9; ++k) printf("%a ", V[k / 3][k % 3]);
            for (int k = 0; k < 9; ++k) printf("%a%c", R1[k / 3][k % 3], k < 8 ? ' ' : '\n');
        } else {
            puts("bad query");
        }
    }
    return 0;
}
