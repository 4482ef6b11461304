// tests/test_deep_rule_host.py: the additive factor rule as the plain kernels have it (cx_scalar_core.h: factor_rule<kRuleAdditive>(m, q, 1, 0),
// two branches, a division in each) and as the deep sweep has it (cx_sweep_deep.hip: deep_rule, one division), restated for the host and
// compared bit for bit, a NaN equal to a NaN.  Built twice by the test, with -ffp-contract=off and =fast: both forms hold the same
// expression 1 + q m.y, so the compiler contracts both or neither.  argv[1]: the number of random inputs.  Prints the count of mismatches.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

struct d2 { double x, y; };

static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }
static double from_bits(uint64_t u) { double v; std::memcpy(&v, &u, 8); return v; }

__attribute__((noinline)) static d2 rule_two_divisions(d2 m, double q) {
    d2 o;
    if (m.y == std::numeric_limits<double>::infinity()) {
        o.y = 1.0 / q;
        o.x = m.x * o.y;
    } else {
        const double s = 1.0 / (1.0 + q * m.y);
        o.y = m.y * s;
        o.x = m.x * s;
    }
    return o;
}

__attribute__((noinline)) static d2 rule_one_division(d2 m, double q) {
    const bool pm = m.y == std::numeric_limits<double>::infinity();
    const double t = from_bits(((pm ? uint64_t(0x3ff00000) : bits(m.y) >> 32) << 32) | (bits(m.y) & 0xffffffffu));
    const double s = 1.0 / ((pm ? -0.0 : 1.0) + q * t);
    return d2{m.x * s, t * s};
}

static bool same(double a, double b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t next() {          // (splitmix64)
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 1000000;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double tiny = std::numeric_limits<double>::denorm_min(), least = std::numeric_limits<double>::min(), most = std::numeric_limits<double>::max();
    const double special[] = {0.0, -0.0, inf, -inf, nan, tiny, -tiny, 1000 * tiny, least, -least, most, -most, 1.0, -1.0, 0.5, 2.0, 1e-12, 1e12, 1e-300, 1e300, 1.0 + 0x1p-52, 3.0};
    const int ns = sizeof special / sizeof *special;
    long bad = 0, checked = 0, point_masses = 0;
    auto check = [&](double x, double y, double q) {
        const d2 a = rule_two_divisions(d2{x, y}, q), b = rule_one_division(d2{x, y}, q);
        checked++;
        point_masses += y == inf;
        if (!same(a.x, b.x) || !same(a.y, b.y)) {
            if (bad++ < 10) std::printf("differ: m = (%a, %a), q = %a: (%a, %a) against (%a, %a)\n", x, y, q, a.x, a.y, b.x, b.y);
        }
    };
    for (int i = 0; i < ns; i++)          // every triple of special values
        for (int j = 0; j < ns; j++)
            for (int k = 0; k < ns; k++) check(special[i], special[j], special[k]);
    for (long i = 0; i < n; i++) {
        // a third: any bit pattern; a third: magnitudes a model has (2^-40 .. 2^40, either sign); a third: one operand special
        double v[3];
        const int kind = (int)(next() % 3);
        for (int k = 0; k < 3; k++) {
            if (kind == 0) v[k] = from_bits(next());
            else v[k] = std::ldexp(1.0 + (double)(next() >> 12) * 0x1p-52, (int)(next() % 81) - 40) * ((next() & 1) ? -1.0 : 1.0);
        }
        if (kind == 2) v[next() % 3] = special[next() % ns];
        if (i % 5 == 0) v[1] = inf;          // the point-mass branch, a fifth of the inputs
        check(v[0], v[1], v[2]);
    }
    std::printf("checked %ld point_masses %ld mismatches %ld\n", checked, point_masses, bad);
    return bad ? 1 : 0;
}
