// Host program for tests/test_switches_host.py: prints the run-time switch table of lattisense_amd/csrc/switches.h and what every
// accessor gives with its variable unset, empty, "0", "1", "2" and "x".
//   ROW <name> <kind> <lifetime>
//   VAL <name> <caller's default or -> <input> <value>     CALL / CONTEXT / PLAN rows: setenv + the accessor itself;
//                                                          PROCESS rows: the uncached parse the accessor calls
//   CACHED <name> <1 if the accessor kept its first value after the variable changed>      PROCESS rows only
// --markdown: the rows of INTEGRATION.md section 6 instead.
#include <cstdio>
#include <initializer_list>

#include "../../lattisense_amd/csrc/switches.h"

using namespace lsa;

static const char* const INPUTS[] = {nullptr, "", "0", "1", "2", "x"};

static void put(const char* name, const char* v) {
    if (v) setenv(name, v, 1);
    else unsetenv(name);
}

template <class Parse, class Read>
static void probe(const sw::Row& r, const char* dflt, Parse parse, Read read) {
    const bool process = !std::strcmp(r.lifetime, "PROCESS");
    for (const char* v : INPUTS) {
        put(r.name, v);
        std::printf("VAL %s %s %s %g\n", r.name, dflt, !v ? "unset" : *v ? v : "empty", process ? parse(v) : read());
    }
    if (process) {
        put(r.name, "0");
        const double first = read();
        put(r.name, "2");
        std::printf("CACHED %s %d\n", r.name, (int)(read() == first));
    }
    put(r.name, nullptr);
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--markdown")) {
        for (const sw::Row& r : sw::table) std::printf("| `%s` | %s | %s |\n", r.name, r.lifetime, r.text);
        return 0;
    }
    for (const sw::Row& r : sw::table) std::printf("ROW %s %s %s\n", r.name, r.kind, r.lifetime);
    int i = 0;
#define PROBE_X(NAME, fn, KIND, LIFE, DESC, ...) \
    probe(sw::table[i++], "-", [](const char* v) { return (double)sw::fn##_of(v); }, [] { return (double)sw::fn(); });
#define PROBE_XD(NAME, fn, KIND, LIFE, DESC, ...)                                                                        \
    for (int d : {0, 5})                                                                                                 \
        probe(sw::table[i], d ? "5" : "0", [d](const char* v) { return (double)sw::fn##_of(v, (sw::KIND##_t)d); }, \
              [d] { return (double)sw::fn((sw::KIND##_t)d); });                                                        \
    i++;
    LSA_SWITCHES(PROBE_X, PROBE_XD)
    return 0;
}
