// HostCells (hemocell_amd/csrc/host_cells.h) on its own: append, stable compaction, sizing for a download, the id-only
// edits and the swap of a built temporary keep the struct's invariants and move every array together.  Cells of nv = 3
// vertices, so a cell is nine doubles per vector array.  Exits 0 when every check holds.
#include "host_cells.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

namespace {
constexpr int NV = 3;
constexpr size_t MARKED = 4;   // the incomplete cell of filled(): tag 2, vertex 1 removed

// every array holds a value that names its array, its cell and its element
double value(int array, size_t cell, size_t k) { return 100.0 * array + 10.0 * (double)cell + (double)k + 0.25; }
long id_of(size_t cell) { return 7000 + 13 * (long)cell; }

void fill_cell(HostCells &H, size_t slot, size_t cell) {
  for (size_t k = 0; k < 3 * NV; k++) {
    const size_t i = 3 * NV * slot + k;
    H.pos[i] = value(1, cell, k); H.vel[i] = value(2, cell, k); H.frc[i] = value(3, cell, k);
    if (H.has_rep) H.rep[i] = value(4, cell, k);
  }
  if (cell == MARKED) { H.tag[slot] = 2; H.dead[NV * slot + 1] = 1; }
}

// the invariant of the struct's head comment, payload held
void check_consistent(const HostCells &H) {
  const size_t n = H.cells() * (size_t)H.nv;
  CHECK(H.pos.size() == 3 * n && H.vel.size() == 3 * n && H.frc.size() == 3 * n);
  CHECK(H.tag.size() == H.cells() && H.dead.size() == n);
  CHECK(H.rep.size() == (H.has_rep ? 3 * n : 0));
}

void check_cell_is(const HostCells &H, size_t slot, size_t cell) {
  CHECK(H.ids[slot] == id_of(cell));
  for (size_t k = 0; k < 3 * NV; k++) {
    const size_t i = 3 * NV * slot + k;
    CHECK(H.pos[i] == value(1, cell, k) && H.vel[i] == value(2, cell, k) && H.frc[i] == value(3, cell, k));
    if (H.has_rep) CHECK(H.rep[i] == value(4, cell, k));
  }
  CHECK(H.tag[slot] == (cell == MARKED ? 2 : 0));
  for (size_t v = 0; v < NV; v++) CHECK(H.dead[NV * slot + v] == ((cell == MARKED && v == 1) ? 1 : 0));
}

void check_cell_is_zero(const HostCells &H, size_t slot) {
  for (size_t k = 0; k < 3 * NV; k++) {
    const size_t i = 3 * NV * slot + k;
    CHECK(H.pos[i] == 0.0 && H.vel[i] == 0.0 && H.frc[i] == 0.0);
    if (H.has_rep) CHECK(H.rep[i] == 0.0);
  }
  CHECK(H.tag[slot] == 0);
  for (size_t v = 0; v < NV; v++) CHECK(H.dead[NV * slot + v] == 0);
}

template <class T>
bool same_prefix(const std::vector<T> &before, const std::vector<T> &after) {
  return after.size() >= before.size() && (before.empty() || std::memcmp(before.data(), after.data(), before.size() * sizeof(T)) == 0);
}

HostCells filled(size_t cells, bool with_rep) {
  HostCells H; H.nv = NV;
  for (size_t c = 0; c < cells; c++) { H.append(id_of(c), with_rep); fill_cell(H, c, c); }
  return H;
}

void test_append(bool with_rep) {
  HostCells H; H.nv = NV;
  CHECK(H.cells() == 0);
  for (size_t c = 0; c < 4; c++) {
    const HostCells before = H;
    H.append(id_of(c), with_rep);
    CHECK(H.cells() == c + 1 && H.has_rep == with_rep);
    check_consistent(H);
    if (!with_rep) CHECK(H.rep.empty());
    // the earlier cells' bytes are untouched in every array, the new cell is zero in every array
    CHECK(same_prefix(before.ids, H.ids) && same_prefix(before.pos, H.pos) && same_prefix(before.vel, H.vel) && same_prefix(before.frc, H.frc));
    CHECK(same_prefix(before.rep, H.rep) && same_prefix(before.tag, H.tag) && same_prefix(before.dead, H.dead));
    CHECK(H.ids[c] == id_of(c));
    check_cell_is_zero(H, c);
    fill_cell(H, c, c == 1 ? MARKED : c);   // one of the earlier cells carries the incomplete mark
    H.ids[c] = id_of(c == 1 ? MARKED : c);
  }
  check_cell_is(H, 0, 0); check_cell_is(H, 1, MARKED); check_cell_is(H, 2, 2); check_cell_is(H, 3, 3);
}

// a repulsion enabled while the payload is held: the cells already here get a zero force_repulsion
void test_append_turns_rep_on() {
  HostCells H = filled(2, false);
  H.append(id_of(2), true);
  CHECK(H.has_rep && H.cells() == 3);
  check_consistent(H);
  for (double r : H.rep) CHECK(r == 0.0);
  H.has_rep = false;   // look at the other arrays of the first two cells only
  check_cell_is(H, 0, 0); check_cell_is(H, 1, 1);
}

void test_compact(bool with_rep) {
  {
    HostCells H = filled(5, with_rep);
    size_t asked = 0;
    const size_t left = H.compact([&](size_t c) { CHECK(c == asked); asked++; return false; });   // once per slot, ascending
    CHECK(left == 0 && asked == 5 && H.cells() == 0);
    check_consistent(H);
  }
  {
    HostCells H = filled(5, with_rep);
    CHECK(H.compact([](size_t) { return true; }) == 5);
    CHECK(H.cells() == 5);
    check_consistent(H);
    for (size_t c = 0; c < 5; c++) check_cell_is(H, c, c);
  }
  {
    HostCells H = filled(5, with_rep);
    CHECK(H.compact([](size_t c) { return c % 2 == 0; }) == 3);
    CHECK(H.cells() == 3);
    check_consistent(H);
    check_cell_is(H, 0, 0); check_cell_is(H, 1, 2); check_cell_is(H, 2, MARKED);   // the incomplete mark followed its cell to slot 2
    H.append(id_of(1), with_rep);   // and the struct goes on working
    check_consistent(H);
    check_cell_is_zero(H, 3);
    check_cell_is(H, 2, MARKED);
  }
}

// hcp_upload_records builds temporaries aside and swaps them in
void test_swap_in(bool with_rep) {
  HostCells H = filled(5, !with_rep);
  HostCells built; built.nv = NV; built.has_rep = with_rep;
  built.append(id_of(3), built.has_rep); fill_cell(built, 0, 3);
  built.append(id_of(MARKED), built.has_rep); fill_cell(built, 1, MARKED);
  std::swap(H, built);
  CHECK(H.cells() == 2 && H.has_rep == with_rep && H.nv == NV);
  check_consistent(H);
  check_cell_is(H, 0, 3); check_cell_is(H, 1, MARKED);
  CHECK(built.cells() == 5 && built.has_rep == !with_rep);
  check_consistent(built);
  for (size_t c = 0; c < 5; c++) check_cell_is(built, c, c);
}

// the device's books change the ids alone; the next download sizes the payload to them
void test_id_only_edits_then_download(bool with_rep) {
  HostCells H = filled(5, with_rep);
  H.ids_push(id_of(5)); H.ids_push(id_of(6));
  H.ids_move(1, 6); H.ids_truncate(6);
  CHECK(H.cells() == 6 && H.ids[0] == id_of(0) && H.ids[1] == id_of(6) && H.ids[2] == id_of(2) && H.ids[5] == id_of(5));
  H.size_payload(!with_rep);
  CHECK(H.has_rep == !with_rep && H.cells() == 6);
  check_consistent(H);
  for (int g : H.tag) CHECK(g == 0);
  for (unsigned char d : H.dead) CHECK(d == 0);
  H.ids_truncate(0);
  H.size_payload(with_rep);
  CHECK(H.cells() == 0);
  check_consistent(H);
}
}  // namespace

int main() {
  for (int with_rep = 0; with_rep < 2; with_rep++) {
    test_append(with_rep != 0);
    test_compact(with_rep != 0);
    test_swap_in(with_rep != 0);
    test_id_only_edits_then_download(with_rep != 0);
  }
  test_append_turns_rep_on();
  std::puts("host_cells ok");
  return 0;
}
