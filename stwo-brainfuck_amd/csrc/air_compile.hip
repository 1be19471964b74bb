// A constraint program compiled to its own gfx950 kernel at run time (include/bfhip.h "Compiled constraint programs"): the source of
// air_codegen.hip goes through hiprtc, the code object through hipModuleLoadData, and bfhip_air_kernel_eval_domain launches it behind the
// checks and the one staged copy of bfhip_air_eval_domain (air_program.hip: air_eval_stage) — same contract, same result to the bit, no
// interpretation. libhiprtc is opened with dlopen at the first compile and never linked: a box without it loses this one entry point and
// nothing else. Nothing is written to disk.
// A context keeps what it compiled (Ctx::air_cache): a module per distinct source, shared by the kernels compiled from equal programs and
// unloaded when the last of them is destroyed. bfhip_ctx_destroy unloads what is left and orphans the kernel objects that still exist:
// they refuse to run and can only be destroyed.
#include "api_guard.h"
#include "air_program.h"
#include "../../include/bfhip.h"
#include <hip/hiprtc.h>
#include <dlfcn.h>
#include <chrono>
#include <mutex>

namespace bf {

struct AirModule {
    u64 hash = 0;
    std::string source;
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    u32 info[7] = {};      // bfhip_air_kernel_info out[0 .. 6]
    u32 users = 0;
};
struct AirKernelCache {
    std::vector<AirModule*> modules;
    std::vector<bfhip_air_kernel*> kernels;
};

}  // namespace bf

struct bfhip_air_kernel {
    bfhip_ctx* ctx = nullptr;      // null once its context is gone
    bf::AirModule* mod = nullptr;
    bfhip_air prog;                // the kernel's own copy: the caller's program may be destroyed
    bool from_cache = false;
};

using namespace bf;

namespace {

std::mutex g_registry;      // the kernel lists of all contexts: a kernel may be destroyed on another thread than its context

// ---- libhiprtc, loaded on first use -----------------------------------------------------------------------------------------------------
struct Hiprtc {
    void* lib = nullptr;
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    decltype(&hiprtcGetErrorString) error_string = nullptr;
};

const Hiprtc& hiprtc() {
    static Hiprtc h;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (h.lib) return h;
    const char* name = "libhiprtc.so.7";
    void* lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    std::string why = lib ? "" : dlerror();
    if (!lib) {      // beside the HIP runtime this library already runs on
        Dl_info di;
        if (dladdr((void*)&hipModuleLoadData, &di) && di.dli_fname) {
            std::string dir(di.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) lib = dlopen((dir.substr(0, slash + 1) + name).c_str(), RTLD_NOW | RTLD_LOCAL);
        }
    }
    if (!lib) throw HipError(std::string("bfhip_air_compile: cannot load ") + name + ": " + why);
    Hiprtc t;
    auto sym = [&](const char* s) {
        void* p = dlsym(lib, s);
        if (!p) { dlclose(lib); throw HipError(std::string("bfhip_air_compile: ") + name + " has no symbol " + s); }
        return p;
    };
    t.create = (decltype(t.create))sym("hiprtcCreateProgram");
    t.compile = (decltype(t.compile))sym("hiprtcCompileProgram");
    t.log_size = (decltype(t.log_size))sym("hiprtcGetProgramLogSize");
    t.log = (decltype(t.log))sym("hiprtcGetProgramLog");
    t.code_size = (decltype(t.code_size))sym("hiprtcGetCodeSize");
    t.code = (decltype(t.code))sym("hiprtcGetCode");
    t.destroy = (decltype(t.destroy))sym("hiprtcDestroyProgram");
    t.error_string = (decltype(t.error_string))sym("hiprtcGetErrorString");
    t.lib = lib;
    h = t;
    return h;
}

u64 fnv1a(const std::string& s) {
    u64 h = 1469598103934665603ull;
    for (unsigned char ch : s) { h ^= ch; h *= 1099511628211ull; }
    return h;
}

// .sgpr_count of the kernel's metadata note (msgpack: the key, then a fixint, uint8 or uint16): hipFuncGetAttribute has no SGPR figure.
// 0xffffffff when the note does not have it.
u32 metadata_count(const std::vector<char>& co, const char* key) {
    const size_t kl = strlen(key);
    for (size_t i = 0; i + kl + 3 <= co.size(); i++) {
        if (memcmp(co.data() + i, key, kl) != 0) continue;
        const unsigned char* v = (const unsigned char*)co.data() + i + kl;
        if (v[0] < 0x80) return v[0];
        if (v[0] == 0xcc) return v[1];
        if (v[0] == 0xcd) return ((u32)v[1] << 8) | v[2];
    }
    return 0xffffffffu;
}

std::vector<char> compile_source(const std::string& source, const std::string& arch) {
    const Hiprtc& rt = hiprtc();
    hiprtcProgram prog = nullptr;
    hiprtcResult r = rt.create(&prog, source.c_str(), "bfhip_air_generated.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) throw HipError(std::string("bfhip_air_compile: hiprtcCreateProgram: ") + rt.error_string(r));
    const std::string target = "--offload-arch=" + arch;
    const char* options[] = {target.c_str(), "-O3", "-std=c++17", "-Wno-pragma-once-outside-header"};
    r = rt.compile(prog, 4, options);
    if (r != HIPRTC_SUCCESS) {
        std::string log;
        size_t n = 0;
        if (rt.log_size(prog, &n) == HIPRTC_SUCCESS && n > 1) { log.resize(n); (void)rt.log(prog, &log[0]); }
        if (log.size() > 1500) log = log.substr(0, 1500) + " ...";
        const std::string what = rt.error_string(r);
        (void)rt.destroy(&prog);
        throw HipError("bfhip_air_compile: hiprtcCompileProgram for " + arch + ": " + what + ": " + log);
    }
    size_t n = 0;
    std::vector<char> co;
    r = rt.code_size(prog, &n);
    if (r == HIPRTC_SUCCESS) { co.resize(n); r = rt.code(prog, co.data()); }
    (void)rt.destroy(&prog);
    if (r != HIPRTC_SUCCESS || co.empty()) throw HipError(std::string("bfhip_air_compile: no code object: ") + rt.error_string(r));
    return co;
}

void release_module(AirKernelCache& cache, AirModule* m) {
    for (size_t i = 0; i < cache.modules.size(); i++) if (cache.modules[i] == m) { cache.modules.erase(cache.modules.begin() + i); break; }
    if (m->module) (void)hipModuleUnload(m->module);
    delete m;
}

}  // namespace

// Ctx::destroy: the stream has been waited for. Unload every module; the kernel objects that still exist lose their context.
void bf::air_kernels_drop(Ctx& c) {
    std::lock_guard<std::mutex> lock(g_registry);
    if (!c.air_cache) return;
    for (bfhip_air_kernel* k : c.air_cache->kernels) { k->ctx = nullptr; k->mod = nullptr; }
    for (AirModule* m : c.air_cache->modules) { if (m->module) (void)hipModuleUnload(m->module); delete m; }
    delete c.air_cache;
    c.air_cache = nullptr;
}

const bfhip_air& bf::air_kernel_program(bfhip_ctx* ctx, bfhip_air_kernel* kernel, const std::string& me) {
    if (kernel->ctx != ctx || !kernel->mod) throw HipError(me + ": the kernel was compiled by another context (a module belongs to the context that loaded it)");
    return kernel->prog;
}

void bf::air_kernel_launch(Ctx& c, bfhip_air_kernel* kernel, const AirLaunch* d_launch, uint32_t n_rows) {
    void* args[] = {(void*)&d_launch};
    ProfScope ps(c.stream, AIR_KERNEL_NAME, 0);
    BF_HIP(hipModuleLaunchKernel(kernel->mod->fn, (n_rows + AIR_KERNEL_LANES - 1) / AIR_KERNEL_LANES, 1, 1, AIR_KERNEL_LANES, 1, 1, 0, c.stream, args, nullptr));
}

extern "C" {

int32_t bfhip_air_compile(bfhip_ctx* ctx, const bfhip_air* air, bfhip_air_kernel** out) {
    API_CTX(ctx)
    if (!air || !out) throw HipError("null argument");
    Ctx& c = ctx->c;
    const auto t0 = std::chrono::steady_clock::now();
    std::string source = air_generate_source(*air);
    const u64 hash = fnv1a(source);
    std::unique_ptr<bfhip_air_kernel> k(new bfhip_air_kernel());
    k->ctx = ctx; k->prog = *air;
    std::lock_guard<std::mutex> lock(g_registry);
    if (!c.air_cache) c.air_cache = new AirKernelCache();
    AirKernelCache& cache = *c.air_cache;
    for (AirModule* m : cache.modules) if (m->hash == hash && m->source == source) { k->mod = m; k->from_cache = true; break; }
    if (!k->mod) {
        hipDeviceProp_t props;
        BF_HIP(hipGetDeviceProperties(&props, c.device));
        const std::vector<char> co = compile_source(source, props.gcnArchName);      // the architecture string as the device reports it
        std::unique_ptr<AirModule> m(new AirModule());
        BF_HIP(hipModuleLoadData(&m->module, co.data()));
        try {
            BF_HIP(hipModuleGetFunction(&m->fn, m->module, AIR_KERNEL_NAME));
            int vgprs = 0, scratch = 0, lds = 0;
            BF_HIP(hipFuncGetAttribute(&vgprs, HIP_FUNC_ATTRIBUTE_NUM_REGS, m->fn));
            BF_HIP(hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, m->fn));
            BF_HIP(hipFuncGetAttribute(&lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, m->fn));
            m->info[0] = (u32)vgprs; m->info[1] = metadata_count(co, ".sgpr_count"); m->info[2] = (u32)scratch; m->info[3] = (u32)lds;
            m->info[4] = (u32)co.size(); m->info[5] = (u32)source.size();
        } catch (...) { (void)hipModuleUnload(m->module); throw; }
        m->info[6] = (u32)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        m->hash = hash; m->source = std::move(source);
        cache.modules.push_back(m.get());
        k->mod = m.release();
    }
    k->mod->users++;
    cache.kernels.push_back(k.get());
    *out = k.release();
    return 0;
    API_CATCH
}

int32_t bfhip_air_kernel_eval_domain(bfhip_ctx* ctx, bfhip_air_kernel* kernel, uint32_t log_size, uint32_t log_expand, const uint32_t* const* cols_h,
                                     const uint32_t* col_shifts_h, const uint32_t* params_h, uint32_t n_params, const uint32_t* coeffs_h, uint32_t n_coeffs,
                                     uint32_t* const acc_d[4]) {
    API_CTX(ctx)
    if (!kernel) throw HipError("null argument");
    const bfhip_air& prog = air_kernel_program(ctx, kernel, "bfhip_air_kernel_eval_domain");
    Ctx& c = ctx->c;
    const AirLaunch* d_launch = air_eval_stage(c, &prog, false, log_size, log_expand, cols_h, col_shifts_h, params_h, n_params, coeffs_h, n_coeffs, acc_d);
    air_kernel_launch(c, kernel, d_launch, 1u << (log_size + log_expand));
    return 0;
    API_CATCH
}

int32_t bfhip_air_kernel_info(bfhip_air_kernel* kernel, uint32_t out[8]) {
    API_TRY
    if (!kernel || !out) throw HipError("null argument");
    std::lock_guard<std::mutex> lock(g_registry);
    if (!kernel->mod) throw HipError("bfhip_air_kernel_info: the kernel's context has been destroyed");
    memcpy(out, kernel->mod->info, sizeof kernel->mod->info);
    out[7] = kernel->from_cache ? 1u : 0u;
    return 0;
    API_CATCH
}

int32_t bfhip_air_kernel_destroy(bfhip_air_kernel* kernel) {
    API_TRY
    if (!kernel) return 0;
    {
        std::lock_guard<std::mutex> lock(g_registry);
        if (kernel->ctx && kernel->mod) {
            Ctx& c = kernel->ctx->c;
            AirKernelCache& cache = *c.air_cache;
            for (size_t i = 0; i < cache.kernels.size(); i++) if (cache.kernels[i] == kernel) { cache.kernels.erase(cache.kernels.begin() + i); break; }
            if (--kernel->mod->users == 0) {      // the last user: no launch of this module may still be running when it is unloaded
                c.bind();
                c.sync();
                release_module(cache, kernel->mod);
            }
        }
    }
    delete kernel;
    return 0;
    API_CATCH
}

}  // extern "C"
