// carmel_output.cpp — the files the front end writes: --write-loaded, the forest-em side files (--fem-*), <member>.trained and
// the single trained transducer (-F or stdout).
#include "carmel_cli.hpp"
#include "fem_export.hpp"
#include "refhash.hpp"
using namespace carmel_host;

void write_loaded(const Job& j) {  // cascade.h:23-32
  const Options& o = j.o;
  for (size_t i = 0; i < j.nw; ++i) {
    std::string fn = trained_path(o.files[i + 1], o.write_loaded);
    std::cerr << "Writing " << o.write_loaded << ' ' << o.files[i + 1] << " to " << fn << std::endl;
    std::ofstream of(fn.c_str());
    of << j.member[i].to_text(o.flags[(unsigned)'J'], o.flags[(unsigned)'H'], j.wstyle);
  }
}

void write_fem_forest(Job& j) {  // cached_derivs.h:44-50, 60-100: written on the first pass over the derivations
  const Options& o = j.o;
  const HostPairs& pairs = j.pairs;
  carmel_host::FemExport fe;
  fe.n_states = (uint32_t)j.result->states.size();
  fe.final_state = j.result->final_state;
  fe.src = &j.src;
  fe.dst = &j.dst;
  fe.in = &j.in;
  fe.out = &j.out;
  fe.group = &j.group;
  fe.chains = j.cascade ? &j.chains.chains : nullptr;
  std::ofstream of(o.fem_forest.c_str());
  if (!of) throw std::runtime_error("could not create --fem-forest=" + o.fem_forest);
  fe.write_forests(of, pairs.size(), pairs.in_off.data(), pairs.in_sym.data(), pairs.out_off.data(), pairs.out_sym.data(),
                   pairs.weight.data());
}

// cascade.h:99-115 over NormGroupIter (fst.h:1362-1446): JOINT -- a group per state, arcs or not, arcs in list order;
// CONDITIONAL -- per state the input symbols in the order the walk over State::index visits them (refhash.hpp), a
// symbol's arcs in reversed list order (state.h:158-199 pushes each onto the front of its symbol's list); NONE -- no groups
void for_each_norm_group(const Transducer& m, int norm, const std::function<void(size_t, const std::vector<size_t>&)>& f) {
  size_t first = 0;
  for (uint32_t s = 0; s < m.states.size(); ++s) {
    const auto& arcs = m.states[s];
    if (norm == CARMEL_HIP_NORM_JOINT) {
      std::vector<size_t> g(arcs.size());
      for (size_t k = 0; k < g.size(); ++k) g[k] = k;
      f(first, g);
    } else if (norm == CARMEL_HIP_NORM_CONDITIONAL && !arcs.empty()) {
      std::vector<uint32_t> syms;
      for (auto& a : arcs) syms.push_back(a.in);
      for (uint32_t sym : carmel_host::conditional_group_order(syms)) {
        std::vector<size_t> g;
        for (size_t k = arcs.size(); k-- > 0;)
          if (arcs[k].in == sym) g.push_back(k);
        f(first, g);
      }
    }
    first += arcs.size();
  }
}

// forest-em side files (carmel.cc:818-831 fem_out; cascade.h:60-116, 167-178)
void write_fem_side_files(Job& j) {
  const Options& o = j.o;
  if (o.fem_norm.empty() && o.fem_alpha.empty() && o.fem_param.empty()) return;
  std::vector<double> all_w(j.n_params());
  hip_check(carmel_hip_get_weights(j.t, all_w.data()), "carmel_hip_get_weights");
  const std::vector<const Transducer*> mem = j.members();
  if (!o.fem_param.empty()) {
    std::cerr << "Writing cascade weights to --fem-param=" << o.fem_param << std::endl;
    std::ofstream of(o.fem_param.c_str());
    for (double w : all_w) of << format_weight(w, W_SOMETIMES_LOG) << "\n";
  }
  if (!o.fem_norm.empty()) {
    std::cerr << "Writing forest-em normgroups to --fem-norm=" << o.fem_norm << std::endl;
    std::ofstream of(o.fem_norm.c_str());
    of << "(";
    uint64_t id0 = 1;
    for (size_t i = 0; i < mem.size(); ++i) {
      of << "\n";
      for_each_norm_group(*mem[i], j.norms[i], [&](size_t first, const std::vector<size_t>& g) {
        of << '(';
        for (size_t k : g) of << ' ' << id0 + first + k;
        of << " )\n";
      });
      id0 += mem[i]->num_arcs();
    }
    of << ")\n";
  }
  if (!o.fem_alpha.empty()) {
    std::cerr << "Writing forest-em alpha to --fem-alpha=" << o.fem_alpha << std::endl;
    std::ofstream of(o.fem_alpha.c_str());
    for (size_t i = 0; i < mem.size(); ++i) {
      const double prior = j.norms[i] == CARMEL_HIP_NORM_NONE ? -1.0 : j.addc[i];
      for (auto& st : mem[i]->states)
        for (auto& a : st) of << (a.group == kLocked ? -1.0 : prior) << '\n';
    }
  }
}

// cm.write_trained("trained") (carmel.cc:1435-1437; cascade.h:23-32): every input transducer with its share of the weights pw
void write_trained_members(Job& j, const double* pw) {
  const Options& o = j.o;
  for (size_t i = 0; i < j.nw; ++i) {
    j.member[i].set_weights(pw + (j.cascade ? j.params.member_base[i] : 0));
    std::string fn = trained_path(o.files[i + 1], "trained");
    std::cerr << "Writing trained " << o.files[i + 1] << " to " << fn << std::endl;
    std::ofstream of(fn.c_str());
    of << j.member[i].to_text(o.flags[(unsigned)'J'], o.flags[(unsigned)'H'], j.wstyle);
  }
}

// the trained single transducer to -F file or stdout (carmel.cc:1485-1496)
int write_single(Job& j) {
  const Options& o = j.o;
  std::vector<double> w(j.logw.size());
  hip_check(carmel_hip_get_weights(j.t, w.data()), "carmel_hip_get_weights");
  j.result->set_weights(w.data());
  std::string txt = j.result->to_text(o.flags[(unsigned)'J'], o.flags[(unsigned)'H'], j.wstyle);
  if (!o.out_file.empty()) {
    std::ofstream of(o.out_file.c_str());
    if (!of) {
      std::cerr << "Could not create file " << o.out_file << ".\n";
      return -8;
    }
    of << txt;
  } else
    std::cout << txt;
  return 0;
}
