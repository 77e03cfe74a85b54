// The run-state kernel's body (catfish_amd/csrc/validation_runs.hpp), stated serially over catfish_amd/csrc/
// validation_runs_word.hpp: a stand-alone program that tests/test_run_states_replay.py builds with g++ -fsanitize=address,
// undefined and holds to device_validation.run_states_host.  Batch file, walk and output: validation_replay_common.hpp.
//
//   validation_runs_replay <batch file> <piece in words> [edge ...]          -> two lines of (edges + 1) * 3 counts, [bin][state]
#include "validation_replay_common.hpp"

#include "../../catfish_amd/csrc/validation_runs_word.hpp"

int main(int argc, char** argv) {
    if (argc < 3 || argc > 3 + CF_RUN_MAX_EDGES) return 2;
    vr_rule rule;
    for (int j = 0; j < CF_RUN_MAX_EDGES; ++j) rule.edges.e[j] = 3 + j < argc ? (unsigned)strtoul(argv[3 + j], nullptr, 10) : 0xffffffffu;
    return replay(argv[1], rule, atoll(argv[2]), (argc - 2) * 3, false);
}
