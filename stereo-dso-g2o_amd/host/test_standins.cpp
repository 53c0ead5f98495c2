// The part of the stand-ins that owns memory, on the CPU alone (no shim, no device library): WindowGraph builds a small window it wrote
// itself, then EnergyFunctional::dropResidual / removePoint / dropPointsF run and the index invariants are checked after every step.
// tests/test_standins_cpu.py compiles and runs it; built with -fsanitize=address,undefined it also shows double deletes, uses after
// removePoint and leaks.
//   test_standins          prints "standins ok"
#include <filesystem>
#include "driver_io.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "test_standins.cpp:%d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

template <class T>
static void put(const std::string& dir, const std::string& name, const std::vector<T>& v) {
  std::ofstream f(dir + "/" + name + ".bin", std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

// 3 frames, 12 points (4 per host), 30 residuals: three per point (targets 0, 1, 2), two for every fourth point, none for point 5
static void write_window(const std::string& dir) {
  const int nf = 3, np = 12, w = 4, h = 2;
  std::vector<int> host, res_point, res_target;
  for (int p = 0; p < np; p++) {
    host.push_back(p / 4);
    for (int t = 0; t < (p == 5 ? 0 : p % 4 == 3 ? 2 : 3); t++) { res_point.push_back(p); res_target.push_back(t); }
  }
  const int nr = (int)res_point.size();
  put(dir, "meta", std::vector<int>{nf, np, nr, w, h, 1, 0});
  put(dir, "calib", std::vector<double>{100, 100, 2, 1, 100, 100, 2, 1});
  std::vector<double> evalPT;
  for (int f = 0; f < nf; f++) for (int i = 0; i < 12; i++) evalPT.push_back(i % 4 == 0 && i < 9 ? 1.0 : i == 9 ? 0.1 * f : 0.0);
  put(dir, "evalPT", evalPT); put(dir, "state", std::vector<double>(nf * 10, 0.0)); put(dir, "state_zero", std::vector<double>(nf * 10, 0.0));
  put(dir, "ab_exposure", std::vector<float>(nf, 1.f)); put(dir, "frameEnergyTH", std::vector<float>(nf, 100.f)); put(dir, "frameID", std::vector<int>{0, 1, 2});
  for (int f = 0; f < nf; f++) put(dir, "img" + std::to_string(f) + "_l0", std::vector<float>((size_t)3 * w * h, 1.f));
  put(dir, "host", host); put(dir, "res_point", res_point); put(dir, "res_target", res_target); put(dir, "res_state", std::vector<uint8_t>(nr, 0));
  for (const char* k : {"u", "v", "idepth", "idepth_zero"}) put(dir, k, std::vector<float>(np, 1.f));
  put(dir, "color", std::vector<float>(np * 8, 1.f)); put(dir, "weights", std::vector<float>(np * 8, 1.f)); put(dir, "hasDepthPrior", std::vector<uint8_t>(np, 0));
}

// residualsAll[k]->idxInAll == k, points[k]->idxInPoints == k, the counters equal what the lists hold, a dropped residual is unlinked
static void check(const WindowGraph& G, const std::vector<PointFrameResidual*>& dropped) {
  int n_points = 0, n_res = 0;
  for (EFFrame* f : G.effs)
    for (size_t k = 0; k < f->points.size(); k++) {
      EFPoint* p = f->points[k];
      REQUIRE(p->idxInPoints == (int)k && p->host == f && p->data->efPoint == p);
      REQUIRE(p->data->residuals.size() == p->residualsAll.size());
      for (size_t i = 0; i < p->residualsAll.size(); i++) {
        EFResidual* r = p->residualsAll[i];
        REQUIRE(r->idxInAll == (int)i && r->point == p && r->data->efResidual == r && r->data->point == p->data);
      }
      n_points++; n_res += (int)p->residualsAll.size();
    }
  REQUIRE(G.ef.nPoints == n_points && G.ef.nResiduals == n_res);
  for (PointFrameResidual* pfr : dropped) REQUIRE(pfr->efResidual == nullptr);
}

// ef->dropResidual, then what FullSystem does with the PointFrameResidual (deleteOut, FullSystem.h:62-71)
static void drop(WindowGraph& G, PointHessian* ph, size_t k) {
  PointFrameResidual* pfr = ph->efPoint->residualsAll[k]->data;
  G.ef.dropResidual(pfr->efResidual);
  auto& l = ph->residuals;
  l.erase(std::find(l.begin(), l.end(), pfr));
  check(G, {pfr});
  delete pfr;
}

int main() {
  char tmpl[] = "/tmp/test_standins_XXXXXX";
  REQUIRE(mkdtemp(tmpl) != nullptr);
  const std::string dir = tmpl;
  write_window(dir);
  {
    WindowGraph G;
    G.build(dir, WindowGraph::Options());
    REQUIRE(G.ef.frames.size() == 3 && G.ef.nPoints == 12 && G.ef.nResiduals == 30 && G.phs[5]->residuals.empty());
    REQUIRE(G.phs[0]->lastResiduals[0].first == G.pfrs[2] && G.phs[0]->lastResiduals[1].first == G.pfrs[1]);
    check(G, {});
    drop(G, G.phs[0], 0);                                          // first: the last entry takes slot 0
    drop(G, G.phs[1], 1);                                          // middle
    drop(G, G.phs[2], 2);                                          // last: nothing moves
    REQUIRE(G.ef.nResiduals == 27 && G.phs[0]->efPoint->residualsAll[0]->data->id == 2);
    G.ef.removePoint(G.phs[9]->efPoint);                           // the second of frame 2's four: point 11 takes its slot
    REQUIRE(G.phs[9]->efPoint == nullptr && G.phs[9]->residuals.empty() && G.effs[2]->points[1]->data->id == 11);
    check(G, {});
    for (int p : {4, 5, 6, 7, 8, 10}) G.phs[p]->efPoint->stateFlag = PS_DROP;   // all of frame 1 (one without residuals); in frame 2 slot 0 and the point that refills it
    G.ef.dropPointsF();
    check(G, {});
    REQUIRE(G.effs[0]->points.size() == 4 && G.effs[1]->points.empty() && G.effs[2]->points.size() == 1 && G.effs[2]->points[0]->data->id == 11);
    REQUIRE(G.ef.nPoints == 5 && G.ef.nResiduals == 27 - 3 - 8 - 6);
  }
  std::filesystem::remove_all(dir);
  std::printf("standins ok\n");
  return 0;
}
