// The switch table of switches.h: its reader and the public query.  The only file of the library that reads the environment;
// compiled once (no IEEE-half twin), so the main objects and their twins see the same values.
#include "switches.h"
#include "../../include/ffm_hip.h"
#include <cstdlib>
#include <cstring>

namespace {

int sw_o0(const char* s) { return s[0] == '0' || (s[0] == 'o' && s[1] != 'n'); }
int sw_o(const char* s) { return s[0] == 'o'; }
int sw_not0(const char* s) { return s[0] != '0'; }
int sw_int(const char* s) { return atoi(s); }
int sw_oint(const char* s) { return s[0] == 'o' ? -1 : atoi(s); }
int sw_vgen(const char* s) { return s[0] == 'v' && s[1] >= '1' && s[1] <= '3' ? s[1] - '0' : 0; }
int sw_4(const char* s) { return s[0] == '4' ? 4 : 2; }

ffm_switches read_switches() {
    ffm_switches sw;
#define X(field, var, rule, dflt, doc) { const char* s = getenv(var); sw.field = s ? rule(s) : (dflt); }
    FFM_SWITCH_TABLE(X)
#undef X
    return sw;
}

}  // namespace

const ffm_switches& ffm_sw() {
    static const ffm_switches sw = read_switches();
    return sw;
}

extern "C" int ffm_switch(const char* name, int* value) {
    if (!name || !value) return FFM_EINVAL;
#define X(field, var, rule, dflt, doc) if (!strcmp(name, var)) { *value = ffm_sw().field; return FFM_OK; }
    FFM_SWITCH_TABLE(X)
#undef X
    return FFM_EINVAL;
}
