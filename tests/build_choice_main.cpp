// The CPU side of tests/test_build_choice.py: pigs_amd/csrc/build_choice.h behind a text protocol, no GPU.
// Compiled by the test with `hipcc -x hip --cuda-host-only`; reads commands from stdin, one per line:
//   L N M c                                  -> the layouts' numbers the launch formulas use
//   C <8 request bools> order N M c q_max q_max_b  <6 settings>  coarse rf box_ok trust takes_strips
//                                            -> choose_build's flags, then its launches
//   O <cmd> ... / P <cmd> ...                -> OrderState / PointsState: set fields, absorb words, ask; prints the state
#include "../pigs_amd/csrc/build_choice.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace pigs;

static float as_float(const std::string& s) { return s == "nan" ? __builtin_nanf("") : s == "inf" ? __builtin_inff() : s == "-inf" ? -__builtin_inff() : std::stof(s); }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main() {
    OrderState o;
    PointsState p;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, sub, tok;
        in >> cmd;
        if (cmd == "L") {
            int64_t N, M; int c;
            in >> N >> M >> c;
            const SamplesLayout s = make_samples_layout(M);
            const PlanLayout pl = make_plan_layout(N > 0 ? N : 1, M, c);
            printf("%u %u %u %u %u %u %u\n", s.scan_blocks, s.h_scan_blocks, s.h_wgs, s.h_chunk, s.cells_per_bin, s.ntiles, pl.scan_blocks);
        } else if (cmd == "C") {
            BuildRequest r; BuildEnv e; MemoryAnswer m;
            std::string q, qb;
            in >> r.do_samples >> r.do_plan >> r.plan_ws_clean >> r.no_lookback >> r.build_lists >> r.defer_lists >> r.fwd_only >> r.order
               >> r.N >> r.M >> r.c >> q >> qb;
            r.q_max = as_float(q); r.q_max_b = as_float(qb);
            in >> e.lattice >> e.lattice_trust >> e.samples_order >> e.gauss_strips >> e.bbox_blocks >> e.no_ahead;
            in >> m.coarse >> m.rf >> m.box_ok >> m.trust >> m.takes_strips;
            const SamplesLayout s = make_samples_layout(r.M);
            PlanLayout pl{};
            if (r.do_plan) pl = make_plan_layout(r.N > 0 ? r.N : 1, r.M, r.c);
            const BuildChoice b = choose_build(r, s, pl, e, m);
            printf("%d %d %u %u %d %d %d %d %d %d %u %.9g %d", b.coarse, b.no_lattice, b.rf_hint, b.bbox_blocks, b.fwd_only, b.ahead,
                   b.s_scan_in_scatter, b.sort_in_count, b.strips, b.trusted, b.s_blocks, b.q_max_b, b.n);
            for (int i = 0; i < b.n; ++i) printf(" %u:%u:%u:%u", (unsigned)b.launches[i].kernel, b.launches[i].grid, b.launches[i].block, b.launches[i].lds);
            printf("\n");
        } else if (cmd == "O") {
            in >> sub;
            int answer = -1;
            if (sub == "reset") o = OrderState{};
            else if (sub == "set") in >> o.rf >> o.same >> o.streak >> o.box_stable;
            else if (sub == "absorb") {      // box (4 floats), runs, points, axis, rf
                uint32_t w[ORDER_WORDS] = {};
                for (int k = 0; k < 4; ++k) { in >> tok; w[k] = bits(as_float(tok)); }
                in >> w[10] >> w[11] >> w[13] >> w[14];
                o.absorb(w);
            } else if (sub == "turn") o.turn_around();
            else if (sub == "trusts") { int mode; in >> mode; answer = o.trusts(mode); }
            else if (sub == "due") { uint32_t nth; in >> nth; answer = o.copy_due(nth); }
            printf("%d %d %u %u %d %d %u %u %u\n", answer, o.coarse, o.rf, o.axis, o.box_seen, o.box_stable, o.same, o.streak, o.broken);
        } else if (cmd == "P") {
            in >> sub;
            int answer = -1;
            if (sub == "reset") p = PointsState{};
            else if (sub == "set") in >> p.strips >> p.same;
            else if (sub == "absorb") {      // n_points, cover, strips, points_wanted, lattice_broken
                uint32_t w[POINTS_WORDS] = {};
                in >> w[0] >> tok >> w[2] >> w[3] >> w[4];
                w[1] = bits(as_float(tok));
                answer = p.absorb(w);
            } else if (sub == "takes") answer = p.takes_strips();
            else if (sub == "due") { uint32_t nth; int trusted; in >> nth >> trusted; answer = p.copy_due(nth, trusted != 0); }
            printf("%d %d %.9g %d %u\n", answer, p.has_points, p.cover, p.strips, p.same);
        }
    }
    return 0;
}
