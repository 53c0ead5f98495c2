// CPU check of plan_activated_stage7 (ba_layout.h): the integers sdso_ba_window_update_activated plans for stage 7, from the integer members
// of activation records.  Stand-alone: includes only ba_layout.h, links nothing of the library.  tests/test_window_activated_cpu.py builds it,
// feeds it the records of the CPU statement and compares what it prints with the NumPy rule:
//   g++ -std=c++17 -O1 test_act_stage7.cpp -o test_act_stage7 && ./test_act_stage7 < case.txt
// and once under the sanitizers (clean when this file was written):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined test_act_stage7.cpp -o test_act_stage7_san
// Input (whitespace separated ints): nf n_add_frames n_remove_frames remove_frames.. nf_act act_frame.. n_rec, then per record
// frame status res_state[0..7].  Output: "refused <why>" or the lines pt_host / rec / res_point / res_target / res_state.
#include "ba_layout.h"
#include <cstdio>
#include <cstring>

static bool rd(int& v) { return std::scanf("%d", &v) == 1; }

int main() {
  int nf, n_add, n_rem, nf_act, n_rec;
  if (!rd(nf) || !rd(n_add) || !rd(n_rem) || n_rem < 0 || n_rem > 64) return 2;
  std::vector<int> rem(n_rem);
  for (int& f : rem) if (!rd(f)) return 2;
  if (!rd(nf_act) || nf_act < 0 || nf_act > 8) return 2;
  std::vector<int> act(nf_act);
  for (int& f : act) if (!rd(f)) return 2;
  if (!rd(n_rec) || n_rec < 0 || n_rec > (1 << 20)) return 2;
  std::vector<sdso::ImmActRec> R(n_rec);
  if (n_rec) std::memset(R.data(), 0, sizeof(sdso::ImmActRec) * R.size());
  for (sdso::ImmActRec& r : R) {
    int st, s;
    if (!rd(r.frame) || !rd(st)) return 2;
    r.status = (int8_t)st;
    for (int k = 0; k < 8; k++) { if (!rd(s)) return 2; r.res_state[k] = (uint8_t)s; }
  }
  sdso_ba_window_edit_t E;
  std::memset(&E, 0, sizeof(E));
  E.n_add_frames = n_add; E.n_remove_frames = n_rem; E.remove_frames = rem.data();
  ActStage7 S;
  const char* why = nullptr;
  if (!plan_activated_stage7(nf, E, nf_act, act.data(), n_rec, R.data(), S, &why)) { std::printf("refused %s\n", why); return 0; }
  auto line = [](const char* name, const std::vector<int>& v) { std::printf("%s", name); for (int x : v) std::printf(" %d", x); std::printf("\n"); };
  line("pt_host", S.pt_host); line("rec", S.rec); line("res_point", S.res_point); line("res_target", S.res_target);
  line("res_state", std::vector<int>(S.res_state.begin(), S.res_state.end()));
  return 0;
}
