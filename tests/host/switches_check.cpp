// switches_check.cpp -- stand-alone check of csrc/switches.h on the host (built with ASan + UBSan by tests/test_switches_host.py).
// One mode per process, because a Once row keeps its first read for the life of the process:
//   unset   every row off / null while its variable is unset; a Once row stays off when the variable is set afterwards
//   one     every row on with "1"; a PerCall row follows a later unset, a Once row does not
//   zero    every row with "0": on iff Any; a PerCall row follows a later "1", a Once row does not
//   text    switch_text returns the text as set, and null when unset, for every row
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "switches.h"

using namespace ngpde;

namespace {

int failures = 0;

void check(bool ok, const char *what, const SwitchRow &row) {
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAILED %s: %s\n", row.name, what);
}

bool yes_no(const SwitchRow &row) { return row.on != SwitchOn::Text; }
bool once(const SwitchRow &row) { return row.read == SwitchRead::Once; }

void clear_all() {
  for (const SwitchRow &row : kSwitchRows) unsetenv(row.name);
}

void mode_unset() {
  clear_all();
  for (int i = 0; i < kNumSwitches; ++i) {
    const SwitchRow &row = kSwitchRows[i];
    const Switch s = (Switch)i;
    check(switch_text(s) == nullptr, "text of an unset variable is not null", row);
    if (!yes_no(row)) continue;
    check(!switch_on(s), "on while unset", row);
    setenv(row.name, "1", 1);
    check(switch_on(s) == !once(row), once(row) ? "a Once row followed a later set" : "a PerCall row missed a later set", row);
    unsetenv(row.name);
  }
}

void mode_one() {
  clear_all();
  for (int i = 0; i < kNumSwitches; ++i) {
    const SwitchRow &row = kSwitchRows[i];
    const Switch s = (Switch)i;
    if (!yes_no(row)) continue;
    setenv(row.name, "1", 1);
    check(switch_on(s), "off with 1", row);
    unsetenv(row.name);
    check(switch_on(s) == once(row), once(row) ? "a Once row followed a later unset" : "a PerCall row missed a later unset", row);
  }
}

void mode_zero() {
  clear_all();
  for (int i = 0; i < kNumSwitches; ++i) {
    const SwitchRow &row = kSwitchRows[i];
    const Switch s = (Switch)i;
    if (!yes_no(row)) continue;
    const bool any = row.on == SwitchOn::Any;
    setenv(row.name, "0", 1);
    check(switch_on(s) == any, any ? "an Any row is off with 0" : "a One row is on with 0", row);
    setenv(row.name, "1", 1);
    check(switch_on(s) == (once(row) ? any : true), once(row) ? "a Once row followed a later 1" : "a PerCall row missed a later 1", row);
    unsetenv(row.name);
  }
}

void mode_text() {
  clear_all();
  for (int i = 0; i < kNumSwitches; ++i) {
    const SwitchRow &row = kSwitchRows[i];
    const Switch s = (Switch)i;
    check(switch_text(s) == nullptr, "text of an unset variable is not null", row);
    setenv(row.name, "16", 1);
    const char *t = switch_text(s);
    check(t && std::strcmp(t, "16") == 0, "text is not the value set", row);
    setenv(row.name, "", 1);
    t = switch_text(s);
    check(t && t[0] == '\0', "text of an empty value is not the empty string", row);
    unsetenv(row.name);
    check(switch_text(s) == nullptr, "text after unset is not null", row);
  }
}

}  // namespace

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "unset")) mode_unset();
  else if (!std::strcmp(mode, "one")) mode_one();
  else if (!std::strcmp(mode, "zero")) mode_zero();
  else if (!std::strcmp(mode, "text")) mode_text();
  else {
    std::fprintf(stderr, "usage: switches_check unset|one|zero|text\n");
    return 2;
  }
  std::printf("%d rows, %d failed checks\n", kNumSwitches, failures);
  return failures ? 1 : 0;
}
