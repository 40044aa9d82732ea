// Host check of the pairwise-pass plan (fmi_amd/csrc/fmi_schedule.h plan_stepwise), built and run by
// tests/test_stepwise_plan.py. For every algorithm the stepwise path serves and P = 1..max, 64, 100, 257 and 1000 it
// executes the plan's live steps in order on slots that hold value ids, and checks:
//   - every operand is resident when it is read (an input always is; a step value must sit in its slot);
//   - a step's destination slot holds nothing that is still to be read or is an output;
//   - every output is resident at the end;
//   - the slot count equals the peak number of temporaries live at once, where a step's destination counts as live
//     before its operands are released.
// What is still to be read is counted here, from the program and the outputs alone, not taken from the plan.
// Prints one summary line and exits 0, or prints the first failure and exits 1.
#include "fmi_schedule.h"  // first: the header stands alone

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace sched = fmi::sched;

namespace {

long g_cases = 0, g_steps = 0;
int g_max_slots = 0;

bool fail(const std::string& name, int P, const std::string& what) {
    std::printf("FAIL %s P=%d: %s\n", name.c_str(), P, what.c_str());
    return false;
}

bool run(const std::string& name, const sched::HostProgram& prog, const std::vector<int32_t>& outs) {
    const int P = prog.peers, nv = prog.nvalues();
    if (!prog.ok) return fail(name, P, "schedule construction failed");
    const sched::StepwisePlan plan = sched::plan_stepwise(prog, outs.data(), static_cast<int>(outs.size()));
    if (static_cast<int>(plan.live.size()) != nv || static_cast<int>(plan.slot.size()) != nv)
        return fail(name, P, "the plan's tables do not have one entry per value");
    // this check's own account: which steps the outputs need, and how many needed steps read each value
    std::vector<char> needed(nv, 0), is_out(nv, 0);
    for (int32_t v : outs) needed[v] = is_out[v] = 1;
    for (int st = prog.nsteps - 1; st >= 0; --st)
        if (needed[P + st]) needed[prog.step[st].a] = needed[prog.step[st].b] = 1;
    std::vector<int> reads(nv, 0);
    for (int st = 0; st < prog.nsteps; ++st) {
        if (!needed[P + st]) continue;
        ++reads[prog.step[st].a];
        if (prog.step[st].b != prog.step[st].a) ++reads[prog.step[st].b];
    }
    for (int v = 0; v < nv; ++v) {
        if ((plan.live[v] != 0) != (needed[v] != 0)) return fail(name, P, "value " + std::to_string(v) + ": live flag wrong");
        const bool temp = v >= P && needed[v];
        if (temp != (plan.slot[v] >= 0)) return fail(name, P, "value " + std::to_string(v) + ": slot given or missing wrongly");
        if (plan.slot[v] >= plan.nslots) return fail(name, P, "value " + std::to_string(v) + ": slot beyond the slot count");
    }
    std::vector<int32_t> holds(plan.nslots, -1);  // the value id each slot holds
    auto resident = [&](int32_t v) { return v < P || holds[plan.slot[v]] == v; };
    int live_temps = 0, peak = 0;
    for (int st = 0; st < prog.nsteps; ++st) {
        if (!plan.live[P + st]) continue;
        const int32_t a = prog.step[st].a, b = prog.step[st].b, d = P + st;
        for (int32_t v : {a, b})
            if (!resident(v)) return fail(name, P, "step " + std::to_string(st) + " reads value " + std::to_string(v) + ", which is not resident");
        const int32_t was = holds[plan.slot[d]];
        if (was >= 0 && (is_out[was] || reads[was] > 0))
            return fail(name, P, "step " + std::to_string(st) + " overwrites value " + std::to_string(was) +
                                     (is_out[was] ? ", an output" : ", which is still to be read"));
        holds[plan.slot[d]] = d;
        peak = std::max(peak, ++live_temps);  // the destination is live before the operands are released
        auto release = [&](int32_t v) {
            if (--reads[v] == 0 && v >= P && !is_out[v]) --live_temps;
        };
        release(a);
        if (b != a) release(b);
        ++g_steps;
    }
    for (int32_t v : outs)
        if (!resident(v)) return fail(name, P, "output value " + std::to_string(v) + " is not resident at the end");
    if (plan.nslots != peak)
        return fail(name, P, std::to_string(plan.nslots) + " slots, but at most " + std::to_string(peak) + " temporaries are live at once");
    g_max_slots = std::max(g_max_slots, plan.nslots);
    ++g_cases;
    return true;
}

bool check_all(int P) {
    const sched::HostProgram ar = sched::build_host(sched::kAllreduce, P);
    std::vector<int> ranks = {0, P / 2, P - 1};
    for (int r : ranks)
        if (!run("allreduce rank " + std::to_string(r), ar, {ar.out[r]})) return false;
    for (auto [alg, name] : {std::pair{sched::kReduce, "reduce"}, std::pair{sched::kReduceLtr, "reduce_ltr"}}) {
        const sched::HostProgram prog = sched::build_host(alg, P);
        if (!run(name, prog, {prog.out[0]})) return false;
    }
    for (auto [alg, name] : {std::pair{sched::kScan, "scan"}, std::pair{sched::kScanLtr, "scan_ltr"},
                             std::pair{sched::kReducePartials, "reduce partials"}}) {
        const sched::HostProgram prog = sched::build_host(alg, P);
        if (!run(name, prog, prog.out)) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int max_p = argc > 1 ? std::atoi(argv[1]) : 40;
    std::vector<int> ps;
    for (int p = 1; p <= max_p; ++p) ps.push_back(p);
    for (int p : {64, 100, 257, 1000})
        if (p > max_p) ps.push_back(p);
    for (int p : ps)
        if (!check_all(p)) return 1;
    std::printf("ok: %ld plans, %ld steps executed, largest plan %d slots, P = 1..%d, 64, 100, 257, 1000\n", g_cases, g_steps,
                g_max_slots, max_p);
    return 0;
}
