// Stand-alone sanitizer run of tests/mw_host/minpoly_host.cpp (no Python, no GPU):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o minpoly_host_san minpoly_host.cpp minpoly_san_main.cpp && ./minpoly_host_san
// the batch of "every status" (pi, e, sqrt 2 + sqrt 3, 50, NaN, +-Inf, 0, 1) at every degree and limb count,
// launch cuts 1, 7, 16, and a one-digit run that ends with status 4
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
extern "C" {
int minpoly_plan_host(int, int, int, int, int32_t *);
void *minpoly_open_host(int, int, int, const double *, int, int, double, int);
int minpoly_launch_host(void *, int);
int minpoly_close_host(void *, int, int32_t *, int32_t *, int32_t *, double *, int32_t *);
}
int main() {
    const int n = 10, plane = 12;
    const long double x[n] = {3.14159265358979323846264338327950288L, 2.71828182845904523536028747135266250L, 1.41421356237309504880168872420969808L + 1.73205080756887729352744634150587237L,
                              50.0L, 0.0L, 0.0L, 0.0L, 0.0L, 1.0L, 1099511627689.0L / 1099511627791.0L};
    int bad = 0;
    for (int limbs : {4, 5, 6, 8, 10})
        for (int deg = 1; deg <= 4; deg++)
            for (int cut : {1, 7, 16})
                for (int nd : {1, 6}) {
                    std::vector<double> v((size_t)limbs * plane, 0.5);
                    for (int i = 0; i < n; i++) {
                        long double r = x[i];
                        for (int l = 0; l < limbs && l < 2; l++) { v[(size_t)l * plane + i] = (double)r; r -= (long double)(double)r; }
                        for (int l = 2; l < limbs; l++) v[(size_t)l * plane + i] = 0.0;
                    }
                    v[4] = NAN; v[5] = INFINITY; v[6] = -INFINITY;
                    const int bits = (deg + 1) * 12 - 6, D = deg + 1;
                    int32_t plan[7];
                    minpoly_plan_host(bits, limbs, deg, nd, plan);
                    void *h = minpoly_open_host(limbs, deg, n, v.data(), plane, bits, 1e-15, nd);
                    int running = 1;
                    for (int it = 0; it < plan[4] / cut + 2 && running; it++) running = minpoly_launch_host(h, cut);
                    std::vector<int32_t> rel((size_t)nd * D * plane, -7), status(plane, -7), rung(plane, -7), info(2 * plane, -7);
                    std::vector<double> err(plane, -7.0);
                    minpoly_close_host(h, plane, rel.data(), status.data(), rung.data(), err.data(), info.data());
                    if (running || status[4] != 2 || status[5] != 2 || status[6] != 2 || status[n] != -7 || (deg == 4 && status[3] != 4)) bad++;
                    if (limbs == 5 && cut == 16) {
                        std::printf("limbs %d deg %d nd %d:", limbs, deg, nd);
                        for (int i = 0; i < n; i++) std::printf(" %d", status[i]);
                        std::printf("\n");
                    }
                }
    std::printf("bad = %d\n", bad);
    return bad != 0;
}
