// The crop preparation's shared arithmetic (maskclustering_amd/csrc/mc_crop_plan.hpp) on the CPU: writes
// the bicubic coefficient tables and the level boxes it computes, for tests/test_clip_crops_cpu.py
// to compare with the numpy restatement (tests/clip_crops_restatement.py).  Built by that test:
//   g++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/crop_plan_check.cpp -o crop_plan_check
// Input (stdin), one request per line:
//   T in_size out_size                        -> "T in out ksize", then out_size lines "xmin n k0 .. k(ksize-1)"
//   B left top right bottom H W levels exp    -> "B", then `levels` lines "left top right bottom w h s ox oy"
#include <algorithm>
#include <cstdio>
#include <vector>

#include "mc_crop_plan.hpp"

int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'T') {
            int s, S;
            if (scanf("%d %d", &s, &S) != 2 || s < 1 || S < 1) return 2;
            const int ksize = mc::crop_ksize(s, S);
            printf("T %d %d %d\n", s, S, ksize);
            std::vector<int32_t> row(ksize);
            for (int xx = 0; xx < S; xx++) {
                int32_t xmin = 0;
                std::fill(row.begin(), row.end(), 0);
                const int n = mc::crop_coeff_row(s, S, xx, &xmin, row.data(), 1);
                if (n > ksize) return 3;
                printf("%d %d", xmin, n);
                for (int j = 0; j < ksize; j++) printf(" %d", row[j]);
                printf("\n");
            }
        } else if (kind == 'B') {
            int l, t, r, b, H, W, levels;
            double e;
            if (scanf("%d %d %d %d %d %d %d %lf", &l, &t, &r, &b, &H, &W, &levels, &e) != 8) return 2;
            printf("B\n");
            for (int lv = 0; lv < levels; lv++) {
                int32_t box[4];
                mc::crop_level_box(l, t, r, b, H, W, lv, e, box);
                const mc::CropSquare q = mc::crop_square(box);
                printf("%d %d %d %d %d %d %d %d %d\n", box[0], box[1], box[2], box[3], q.w, q.h, q.s, q.ox, q.oy);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
