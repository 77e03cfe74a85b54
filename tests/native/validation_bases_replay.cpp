// The base kernel's body (catfish_amd/csrc/validation_bases.hpp), stated serially over catfish_amd/csrc/
// validation_bases_word.hpp: a stand-alone program that tests/test_run_bases_replay.py builds with g++ -fsanitize=address,
// undefined and holds to device_validation.run_bases_host.  Batch file (with the base map), walk and output:
// validation_replay_common.hpp.
//
//   validation_bases_replay <batch file> <max_bases> <piece in words>        -> two lines of 3 * 5 * (max_bases + 1) counts
#include "validation_replay_common.hpp"

#include "../../catfish_amd/csrc/validation_bases_word.hpp"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int max_bases = atoi(argv[2]);
    if (max_bases < 1 || max_bases > VBS_MAX_BASES) return 2;
    return replay(argv[1], vbs_rule{max_bases}, atoll(argv[3]), vbs_cells(max_bases), false);
}
