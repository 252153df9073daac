// host_prep_main.cpp -- the stand-alone driver of tests/test_host_prep_cpu.py: raw arrays in, the pure host preparation of the engine
// (pgdrive_amd/csrc/pgd_host_prep.h, no HIP in it), raw results out.  Built by the test with the host compiler and the address and
// undefined-behaviour sanitizers; every input array lives in a heap block of exactly its size, so a read past an array ends the run.
//   geometry  IN OUT                         IN: records {pgd_config, int32 pack, int32 imask}; OUT: records {int32 rc, Geometry}
//   regroup   IN OUT                         IN: records {Geometry, int32 N, n_groups, imask}; OUT: records {int32 rc, Geometry, int32 left}
//   maps      MAPS LANES ROADS BOXES CS CI NULLS PREFIX    NULLS: bit k = array k (in this order) is passed as a null pointer;
//                                            writes PREFIX.lanes / .nav / .cbox / .cext / .cs
//   scen      SCEN SPAWNS SSTRIDE NO_UNI PREFIX            writes PREFIX.spawns
//   state_in  F I EI N V PREFIX              ABI fields -> PREFIX.rec (piece planes), PREFIX.env
//   state_out REC ENV N V PREFIX             piece planes -> PREFIX.f / .i / .ei
//   planes    REC V PREFIX                   records, one after the other -> PREFIX.planes -> PREFIX.back
// Every command prints "rc N" (and what else it returns by value) on stdout; its exit status is 0 unless a file could not be used.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../pgdrive_amd/csrc/pgd_host_prep.h"

template <typename T> static std::vector<T> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (bytes % (long)sizeof(T)) { fprintf(stderr, "%s: %ld bytes is no whole number of %zu-byte records\n", path, bytes, sizeof(T)); exit(2); }
  std::vector<T> v((size_t)bytes / sizeof(T));
  if (bytes && fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "short read of %s\n", path); exit(2); }
  fclose(f);
  v.shrink_to_fit();
  return v;
}
template <typename T> static void write_file(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || (n && fwrite(p, sizeof(T), n, f) != n)) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}
template <typename T> static void write_file(const std::string& path, const std::vector<T>& v) { write_file(path, v.data(), v.size()); }
// an array as the ABI's callers pass it: null when empty, or when the test asks for a null pointer
template <typename T> static const T* arg(const std::vector<T>& v, bool null) { return (null || v.empty()) ? nullptr : v.data(); }

struct GeometryIn { pgd_config cfg; int32_t pack, imask; };
struct GeometryOut { int32_t rc; Geometry g; };
struct RegroupIn { Geometry g; int32_t N, n_groups, imask; };
struct RegroupOut { int32_t rc; Geometry g; int32_t left; };

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "geometry" && argc == 4) {
    const auto in = read_file<GeometryIn>(argv[2]);
    std::vector<GeometryOut> out(in.size());
    for (size_t k = 0; k < in.size(); ++k) {
      out[k].g = Geometry{-1, -1, -1, -1, -1, -1, -1, -1};
      out[k].rc = plan_geometry(in[k].cfg, in[k].pack, in[k].imask, out[k].g);
    }
    write_file(argv[3], out);
  } else if (cmd == "regroup" && argc == 4) {
    const auto in = read_file<RegroupIn>(argv[2]);
    std::vector<RegroupOut> out(in.size());
    for (size_t k = 0; k < in.size(); ++k) {
      bool left = false;
      out[k].rc = regroup_geometry(in[k].g, in[k].N, in[k].n_groups, in[k].imask, out[k].g, &left);
      out[k].left = left ? 1 : 0;
    }
    write_file(argv[3], out);
  } else if (cmd == "maps" && argc == 10) {
    const auto maps = read_file<pgd_map>(argv[2]);
    const auto lanes = read_file<pgd_lane>(argv[3]);
    const auto roads = read_file<pgd_road>(argv[4]);
    const auto boxes = read_file<pgd_box>(argv[5]);
    const auto cs = read_file<int32_t>(argv[6]);
    const auto ci = read_file<int32_t>(argv[7]);
    const int nulls = atoi(argv[8]);
    const std::string prefix = argv[9];
    MapTables t;
    const int rc = build_map_tables(arg(maps, nulls & 1), (int)maps.size(), arg(lanes, nulls & 2), (int)lanes.size(), arg(roads, nulls & 4),
                                    (int)roads.size(), arg(boxes, nulls & 8), (int)boxes.size(), arg(cs, nulls & 16), (int)cs.size(),
                                    arg(ci, nulls & 32), (int)ci.size(), t);
    printf("rc %d\n", rc);
    if (rc == PGD_OK) {
      write_file(prefix + ".lanes", t.lanes.data(), lanes.size());
      write_file(prefix + ".nav", t.nav.data(), lanes.size());
      write_file(prefix + ".cbox", t.cell_boxes.data(), ci.size());
      write_file(prefix + ".cext", t.cell_ext.data(), ci.size());
      write_file(prefix + ".cs", t.cell_start.data(), cs.size());
    }
  } else if (cmd == "scen" && argc == 7) {
    const auto scen = read_file<pgd_scenario>(argv[2]);
    const auto spawns = read_file<pgd_spawn>(argv[3]);
    const int sstride = atoi(argv[4]);
    if (spawns.size() != scen.size() * (size_t)sstride) { fprintf(stderr, "%zu spawn records for %zu scenarios\n", spawns.size(), scen.size()); return 2; }
    ScenarioTables t;
    const int rc = build_scenario_tables(arg(scen, false), arg(spawns, false), (int)scen.size(), sstride, atoi(argv[5]) != 0, t);
    printf("rc %d\n", rc);
    if (rc == PGD_OK) {
      printf("has_objects %d\nno_groups %d\nuni_len %a\nuni_wid %a\n", t.has_objects ? 1 : 0, t.no_groups, (double)t.uni_len, (double)t.uni_wid);
      write_file(std::string(argv[6]) + ".spawns", t.spawns);
    }
  } else if (cmd == "state_in" && argc == 8) {
    const auto f = read_file<float>(argv[2]);
    const auto i = read_file<int32_t>(argv[3]);
    const auto ei = read_file<int32_t>(argv[4]);
    const int N = atoi(argv[5]), V = atoi(argv[6]);
    const size_t nv = (size_t)N * V;
    if (f.size() != PGD_NF * nv || i.size() != PGD_NI * nv || ei.size() != (size_t)PGD_NEI * N) { fprintf(stderr, "state blobs of another size\n"); return 2; }
    std::vector<RecUnit> rec(nv * 8);
    std::vector<int32_t> env((size_t)N * PGD_NEI);
    const int rc = state_from_fields(f.data(), i.data(), ei.data(), N, V, rec.data(), env.data());
    printf("rc %d\n", rc);
    if (rc == PGD_OK) {
      write_file(std::string(argv[7]) + ".rec", rec);
      write_file(std::string(argv[7]) + ".env", env);
    }
  } else if (cmd == "state_out" && argc == 7) {
    const auto rec = read_file<RecUnit>(argv[2]);
    const auto env = read_file<int32_t>(argv[3]);
    const int N = atoi(argv[4]), V = atoi(argv[5]);
    const size_t nv = (size_t)N * V;
    if (rec.size() != nv * 8 || env.size() != (size_t)N * PGD_NEI) { fprintf(stderr, "records of another size\n"); return 2; }
    std::vector<float> f(PGD_NF * nv);
    std::vector<int32_t> i(PGD_NI * nv), ei((size_t)PGD_NEI * N);
    state_to_fields(rec.data(), env.data(), N, V, f.data(), i.data(), ei.data());
    printf("rc %d\n", PGD_OK);
    write_file(std::string(argv[6]) + ".f", f);
    write_file(std::string(argv[6]) + ".i", i);
    write_file(std::string(argv[6]) + ".ei", ei);
  } else if (cmd == "planes" && argc == 5) {
    const auto rec = read_file<VehRec>(argv[2]);
    const int V = atoi(argv[3]);
    if (V <= 0 || rec.size() % (size_t)V) { fprintf(stderr, "%zu records are no whole blocks of %d\n", rec.size(), V); return 2; }
    std::vector<RecUnit> planes(rec.size() * 8);
    std::vector<VehRec> back(rec.size());
    for (size_t k = 0; k < rec.size(); ++k) record_to_planes(planes.data(), V, k, rec[k]);
    for (size_t k = 0; k < rec.size(); ++k) record_from_planes(planes.data(), V, k, back[k]);
    printf("rc %d\n", PGD_OK);
    write_file(std::string(argv[4]) + ".planes", planes);
    write_file(std::string(argv[4]) + ".back", back);
  } else {
    fprintf(stderr, "usage: see the head of tests/host_prep_main.cpp\n");
    return 2;
  }
  return 0;
}
