// seed_san_main.cpp — the cases of tests/hostemu_seed.cpp as a program of its own, for the host sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc \
//       tests/diag/seed_san_main.cpp -o tests/_hostemu/seed_san && tests/_hostemu/seed_san
// Every read of the cases sits in a heap block of exactly its length plus CM_STAGE_PAD bytes on both sides, so a word load of the
// k-mer path that left the slack would be reported.  Exit status 0 = no mismatch against the byte loop and no report.
#include "../hostemu_seed.cpp"

int main(int argc, char **) { return seedw_all(argc > 1) == 0 ? 0 : 1; }
