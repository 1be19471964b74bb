// The error boundary of the C ABI (include/bfhip.h): every extern "C" function that returns int32_t opens with API_TRY, API_CTX(ctx) or
// API_POOL(pool) and closes with API_CATCH — the ONLY place where an exception becomes bfhip_set_error(...) and the return value -1, whatever
// was thrown (nothing may unwind through extern "C"); a bf::TraceRejected (a proof's preflight) becomes BFHIP_TRACE_REJECTED. Codes other than -1 (-2 = "capacity", 1 = proof rejected) are returned by the entry
// points themselves. Device memory of one call is owned by a scope guard (ctx.h: DeviceScratch, ArenaBorrow); other clean-up that has to run
// on failure is an inner `catch (...) { clean up; throw; }` in front of this boundary.
#pragma once
#include "ctx.h"

#define API_TRY try {
#define API_CTX(ctx) try { if (!(ctx)) throw bf::HipError("null context"); (ctx)->c.bind();
#define API_POOL(pool) try { if (!(pool)) throw bf::HipError("null pool");
#define API_CATCH } catch (const bf::TraceRejected& e) { bfhip_set_error(e.what()); return -3; /* BFHIP_TRACE_REJECTED */ } catch (const std::exception& e) { bfhip_set_error(e.what()); return -1; } catch (...) { bfhip_set_error("unknown error"); return -1; }
