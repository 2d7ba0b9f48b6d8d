// compat forwarding header: helper/bindingField.h of the reference.  The binding field is the device lattice's (one byte per
// node, csrc/solidify.hip); bindingFieldHelper edits it site by site.  Coordinates are global node coordinates: the one
// atomic block of this back end is the whole domain.  The field travels in HemoCell::saveCheckPoint / loadCheckPoint, so
// checkpoint() and restore() have nothing left to do.
#pragma once
#include "hemocell.h"
namespace hemo {
class bindingFieldHelper {
 public:
  static bindingFieldHelper &get(HemoCellFields &cellFields) { static bindingFieldHelper instance(&cellFields); return instance; }
  void checkpoint() {}
  static void restore(HemoCellFields &) {}
  void add(HemoCellParticleField &, const plb::Dot3D &site) { set(vector<plb::Dot3D>{site}, 1); }
  void add(HemoCellParticleField &, const vector<plb::Dot3D> &sites) { set(sites, 1); }
  void remove(HemoCellParticleField &, const plb::Dot3D &site) { set(vector<plb::Dot3D>{site}, 0); }
  void remove(HemoCellParticleField &, const vector<plb::Dot3D> &sites) { set(sites, 0); }
  bindingFieldHelper(bindingFieldHelper const &) = delete;
  void operator=(bindingFieldHelper const &) = delete;
 private:
  explicit bindingFieldHelper(HemoCellFields *cellFields_) : cellFields(*cellFields_) {}
  void set(const vector<plb::Dot3D> &sites, uint8_t value) {
    auto *L = cellFields.hemocell.lattice;
    hc_lattice *d = cellFields.bindingDevice();
    vector<uint8_t> field((size_t)L->nx * L->ny * L->nz);
    hc_check(hcl_binding_download(d, field.data()), "hcl_binding_download");
    for (const plb::Dot3D &s : sites) {
      if (s.x < 0 || s.x >= L->nx || s.y < 0 || s.y >= L->ny || s.z < 0 || s.z >= L->nz) continue;
      field[((size_t)s.x * L->ny + (size_t)s.y) * L->nz + (size_t)s.z] = value;
    }
    hc_check(hcl_binding_upload(d, field.data()), "hcl_binding_upload");
  }
  HemoCellFields &cellFields;
};
}  // namespace hemo
