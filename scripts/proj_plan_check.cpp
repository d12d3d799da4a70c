// The projected boxes' shared arithmetic (maskclustering_amd/csrc/mc_proj_plan.hpp) on the CPU: prints
// the status, box and in-bounds count it computes for each request, and the draw clamp, for
// tests/test_top_views_cpu.py to compare with the numpy restatement (tests/top_views_restatement.py).
// Built by that test:
//   g++ -std=c++17 -O1 -g -Wall -Werror -ffp-contract=off -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/proj_plan_check.cpp -o proj_plan_check
// Input (stdin), numbers as C99 hexadecimal floats or inf / nan:
//   P width height n m0 .. m15 fx fy cx cy, then n lines "x y z"  -> "P status x0 y0 x1 y1 inside"
//   C x0 y0 x1 y1 width height thickness                           -> "C x0 y0 x1 y1"
#include <cstdio>

#include "mc_proj_plan.hpp"

int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'P') {
            int width, height, n;
            double m[16], k[4];
            if (scanf("%d %d %d", &width, &height, &n) != 3 || n < 0) return 2;
            for (double &v : m)
                if (scanf("%lf", &v) != 1) return 2;
            for (double &v : k)
                if (scanf("%lf", &v) != 1) return 2;
            mc::ProjAcc a;
            mc::proj_acc_init(&a);
            for (int i = 0; i < n; i++) {
                double x, y, z;
                if (scanf("%lf %lf %lf", &x, &y, &z) != 3) return 2;
                int px = 0, py = 0;
                const int pk = mc::proj_point(m, k, x, y, z, width, height, &px, &py);
                mc::proj_acc_add(&a, pk, px, py);
            }
            int32_t box[4];
            const int st = mc::proj_acc_box(&a, box);
            printf("P %d %d %d %d %d %d\n", st, box[0], box[1], box[2], box[3], st == mc::kProjOk ? a.inside : 0);
        } else if (kind == 'C') {
            int32_t b[4], out[4];
            int width, height, thickness;
            if (scanf("%d %d %d %d %d %d %d", &b[0], &b[1], &b[2], &b[3], &width, &height, &thickness) != 7) return 2;
            mc::proj_draw_clamp(b, width, height, thickness, out);
            printf("C %d %d %d %d\n", out[0], out[1], out[2], out[3]);
        } else {
            return 2;
        }
    }
    return 0;
}
