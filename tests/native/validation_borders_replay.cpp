// The border kernel's body (catfish_amd/csrc/validation_borders.hpp), stated serially over catfish_amd/csrc/
// validation_borders_word.hpp: a stand-alone program that tests/test_run_borders_replay.py builds with g++ -fsanitize=address,
// undefined and holds to device_validation.run_borders_host.  Batch file, walk and output: validation_replay_common.hpp; every
// stretch is walked forward (left offsets, interruptions) and mirrored (right offsets).
//
//   validation_borders_replay <batch file> <reach> <piece in words>          -> two lines of 5 * reach + 3 counts
#include "validation_replay_common.hpp"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int reach = atoi(argv[2]);
    if (reach < 1 || reach > VB_MAX_REACH) return 2;
    return replay(argv[1], vb_rule{reach}, atoll(argv[3]), vb_cells(reach), true);
}
