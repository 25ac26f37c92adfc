// The one place that reads the environment (switches.h has the table and the parse conventions).
#include "switches.h"

#include <cstdlib>

namespace wb {
namespace sw {

static bool read_bool(const char* name, Kind kind) {
  const char* e = getenv(name);
  switch (kind) {
    case OPT_IN: return e && e[0] == '1';
    case UNSET_OR_1: return e ? e[0] == '1' : true;
    default: return !(e && e[0] == '0');
  }
}
static int read_int(const char* name, Kind kind, int dflt) {
  const char* e = getenv(name);
  if (!e) return dflt;
  return kind == TRI ? (e[0] == '0' ? 0 : 1) : atoi(e);
}

// (function-local statics: read at the accessor's first call, once, thread-safe)
#define WB_SW_DEF(fn, name, kind, dflt, what) \
  bool fn() { static const bool v = read_bool(name, kind); return v; }
WB_BOOL_SWITCHES(WB_SW_DEF)
#undef WB_SW_DEF
#define WB_SW_DEF(fn, name, kind, dflt, what) \
  int fn() { static const int v = read_int(name, kind, dflt); return v; }
WB_INT_SWITCHES(WB_SW_DEF)
#undef WB_SW_DEF
#define WB_SW_DEF(fn, name, kind, dflt, what) \
  const char* fn() { static const char* const v = getenv(name); return v; }
WB_STR_SWITCHES(WB_SW_DEF)
#undef WB_SW_DEF

}  // namespace sw
}  // namespace wb
