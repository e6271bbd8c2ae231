// swath_sanitize_driver.cpp -- csrc/fcpp_swathfn.h (the rule behind fcpp_debug_swaths and the polygon swath kernels) under ASan + UBSan on
// the CPU: the comb, the L with its hole, a 300-vertex star, the comb over the crossing cap and a field with a NaN vertex, at random angles,
// widths and offsets.  Any sanitizer report aborts; the driver itself checks what every field must give: records in order inside their
// line, statuses, and the count the totals report.  usage: swath_sanitize_driver SEED N
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../field_coverage_path_planning_amd/csrc/fcpp_swathfn.h"

using namespace fcpp;

struct Field {
    std::vector<int64_t> vo{ 0 };
    std::vector<double> x, y;
    void ring(const std::vector<double> &px, const std::vector<double> &py)
    {
        x.insert(x.end(), px.begin(), px.end());
        y.insert(y.end(), py.begin(), py.end());
        vo.push_back((int64_t)x.size());
    }
};

static Field comb(int teeth)
{
    std::vector<double> px{ 0.0 }, py{ 0.0 };
    double x = 10.0 * (2 * teeth - 1);
    px.push_back(x); py.push_back(0.0);
    for (int t = 0; t < teeth; ++t) {
        px.push_back(x); py.push_back(40.0); px.push_back(x - 10.0); py.push_back(40.0);
        x -= 10.0;
        if (t < teeth - 1) { px.push_back(x); py.push_back(10.0); px.push_back(x - 10.0); py.push_back(10.0); x -= 10.0; }
    }
    Field f;
    f.ring(px, py);
    return f;
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const long n = argc > 2 ? strtol(argv[2], nullptr, 10) : 2000;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    std::vector<Field> fields;
    fields.push_back(comb(4));
    Field ell;
    ell.ring({ 0, 60, 60, 25, 25, 0 }, { 0, 0, 20, 20, 50, 50 });
    ell.ring({ 10, 20, 20, 10 }, { 5, 5, 15, 15 });
    fields.push_back(ell);
    Field star;
    {
        std::vector<double> a(300), px(300), py(300);
        for (double &v : a) v = 6.283185307179586 * unit(rng);
        std::sort(a.begin(), a.end());
        for (int k = 0; k < 300; ++k) { const double r = 40.0 + 80.0 * unit(rng); px[k] = 300.0 + r * cos(a[k]); py[k] = -120.0 + r * sin(a[k]); }
        star.ring(px, py);
    }
    fields.push_back(star);
    fields.push_back(comb(SWATH_MAX_CROSSINGS / 2 + 8));
    Field bad = ell;
    bad.y[2] = NAN;
    fields.push_back(bad);
    Field two = ell;
    two.ring({ 1.0, 2.0 }, { 1.0, 2.0 });
    fields.push_back(two);
    const double widths[4] = { 3.2, 1.0, 0.37, 5.0 };
    long ok = 0, invalid = 0, unsupported = 0, swaths = 0;
    for (long it = 0; it < n; ++it) {
        const Field &f = fields[(size_t)(it % (long)fields.size())];
        const double W = widths[(it / 7) % 4], theta = it % 5 == 0 ? 0.0 : (unit(rng) - 0.5) * 20.0;
        const double first = it % 3 == 0 ? 0.0 : W * unit(rng) * 0.999, min_length = it % 4 == 0 ? 12.0 * unit(rng) : 0.0;
        std::vector<double> u(f.x.size()), w(f.x.size());
        int64_t last_k = -1, count = 0;
        double last_u = 0.0, sum = 0.0;
        bool order = true;
        const SwathTotals t = swath_field_host(f.vo.data(), 0, (int64_t)f.vo.size() - 1, f.x.data(), f.y.data(), theta, W, first, min_length, u.data(),
                                               w.data(), [&](int64_t k, double ua, double ub, double, double, double, double len) {
            if (k < last_k || (k == last_k && ua < last_u) || !(ub - ua > min_length) || len != ub - ua) order = false;
            last_k = k; last_u = ub; ++count; sum += len;
        });
        const int kind = (int)(it % (long)fields.size());
        const int expect = kind == 4 || kind == 5 ? SWATH_EINVAL : SWATH_OK;
        if (!order) { printf("records out of order at %ld\n", it); return 1; }
        if (kind != 3 && t.status != expect) { printf("status %d at %ld\n", t.status, it); return 1; }
        if (t.status != SWATH_OK && (count || t.n_swaths || t.n_lines || t.length != 0.0)) { printf("output with a status at %ld\n", it); return 1; }
        if (t.status == SWATH_OK && (count != t.n_swaths || last_k >= t.n_lines || fabs(sum - t.length) > 1e-9 * (1.0 + sum))) { printf("totals at %ld\n", it); return 1; }
        if (t.status == SWATH_OK) ++ok; else if (t.status == SWATH_EINVAL) ++invalid; else ++unsupported;
        swaths += count;
    }
    printf("ok %ld invalid %ld unsupported %ld swaths %ld\n", ok, invalid, unsupported, swaths);
    return 0;
}
