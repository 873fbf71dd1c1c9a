// aggregator_main.cpp -- drop-in replacement for pipeline_simulation/aggregator.cpp.
//
// Same process role (node id -1), same CLI (-i/-d/-c, aggregator.cpp:13-32),
// same wire protocol and the same round structure (aggregator.cpp:55-167):
//   refactor  <- the init node's REFACTOR_DATA_OWNER message (:52-53)
//   phase 1   <- D receipts of model_part 1, reduced, reply to 0 and i+c+1 (:59-106)
//   phase 2   <- D*L receipts of model_parts 2..L+1, reduced, reply per layer (:108-166)
// What changes is only how a receipt is consumed: frames are received into
// pooled pinned buffers (one reader thread per connection), the archive is
// mapped in place (host/archive.h) and its parameter records are DMA'd straight
// from the frame to the client's device slot (fa_submit_gather_pinned); at the
// end of a phase one ordered FMA chain per bucket runs on the MI355X and the
// result is DMA'd straight into the parameter records of the reply frame
// (fa_finalize_gather).  The reply archive is the last receipt's with the
// reduced parameters (buffers stay the last receipt's, as in the reference),
// built once and sent to every data owner.
//
// Client slots (the FMA chain order) are fixed, not arrival-ordered: the
// refactor message's data-owner list when it has D entries, else the reply
// convention of aggregator.cpp:102-106 (owner ids 0, C+1, ..., C+D-1).
//
// --mode literal reproduces the reference's arithmetic bit-for-bit
// (fl(fl(x_last + x_last) / 1000)); --mode fedavg (default) is
// the north star's weighted mean (weights n_k/N from --samples, else 1/D);
// --mode trimmed [--trim T] / --mode median is the coordinate-wise trimmed
// mean (FA_TRIMMED, fa.h), which T owners sending NaN or inf do not reach.
//
// --server-opt momentum|adagrad|adam|yogi puts a server optimizer (fa.h "Server optimizer") behind the
// aggregate of every bucket: the global model and its moments stay on the GPU in fp32 across rounds, and
// --server-state FILE carries them across restarts.
// --clip-norm C bounds every owner's update (its receipt minus the global model it was last sent) to an L2
// norm of C before the FedAvg chain (fa.h "Clip stage"); --clip-state FILE carries that model across restarts.
// --krum-f F [--krum-m M] averages, per bucket, only the M owners (default D - F) whose receipts lie closest to
// the others' (Krum / Multi-Krum, fa.h "Krum stage"); the stage keeps no state across rounds.
// --geomed-iters T [--geomed-nu NU] replaces, per bucket, the weighted mean by the weighted geometric median of the
// owners' receipts, found by T smoothed Weiszfeld passes (RFA, fa.h "Geomed stage"): nobody is left out, an owner far
// from the others is down-weighted; the stage keeps no state across rounds.
// --mode bulyan --bulyan-f F picks, per bucket, D - 2F owners by iterated Krum and averages per element the picked
// values closest to their median (fa.h "Bulyan stage"); the stage keeps no state across rounds.
// --dp-noise-multiplier Z (with --clip-norm C) adds Gaussian noise of stddev Z C max_k w_k to every bucket's clipped
// aggregate (fa.h "Noise stage"): DP-FedAvg; the seed is fresh entropy at every start unless --dp-seed fixes it.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <fstream>
#include <iostream>
#include <map>
#include <random>
#include <set>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "archive.h"
#include "fedavg/fa.h"
#include "net.h"
#include "receipts.h"

using namespace fahost;

namespace {

struct Options {
    int id = -1, data_owners = 1, compute_nodes = 1;
    int gpus = 1, rounds = -1, port_base = 8079, last_layers = -1;
    fa_mode mode = FA_FEDAVG;
    float divisor = 1000.0f;  // kTrainSize_10, aggregator.cpp:48
    // --mode trimmed [--trim T] / --mode median: FA_TRIMMED, the coordinate-wise trimmed mean (fa.h); the
    // median is its largest trim, (D-1)/2
    int trim = FA_TRIM_MEDIAN;
    bool trim_given = false, median = false;
    // --mode bulyan --bulyan-f F: FA_TRIMMED buckets with the Bulyan stage (fa_set_bulyan on the context, before
    // any bucket is defined): iterated Krum, then per element the mean of the values closest to the median
    int bulyan_f = 0;
    bool bulyan = false, bulyan_f_given = false;
    bool discover = false, pinned = true;
    bool rs = false;     // --layout rs: clients dealt to the GPUs, RCCL reduce-scatter of fp32 partials
    bool eager = false;  // --eager: accumulate on arrival (the chain advances with the in-order receipts)
    // --test-shared-device: the --gpus G shards all on GPU 0 (FA_TEST_SHARED_DEVICE; the rs exchange replaced
    // by its definition), so the multi-GPU layouts run end to end on a one-GPU box (tests only)
    bool shared_device = false;
    int rs_chunks = 0;
    double link_mbps = 0;
    // failure detection: after stall_report_s without a receipt, name the data owners still missing;
    // after receipt_timeout_s (0 = wait forever, the reference's behaviour), give up with exit code 3
    double stall_report_s = 60, receipt_timeout_s = 0;
    // large receipts received at once (NetLayer::set_rx_concurrency; 0 = no limit).  C4 at D = 64 over
    // loopback (gpurun_out r02s40), owner-view round: unlimited 3.15-3.32 s, 4 at a time 2.05-2.48 s,
    // 16 at a time 2.15-2.31 s -- the phase end drops from 0.48-0.51 s to 0.04-0.17 s
    int rx_concurrency = 8;
    int senders = 8;  // fan-out sender threads (each destination keeps to one, in order)
    // streaming ingest: receipt frames of at least this many bytes go to their slot record by record while
    // they arrive (NetLayer::set_streaming; pinned frames only); 0 = off
    size_t stream_min = 1u << 20;
    // --mx8: buckets take MX8 receipts (fa_set_mx8 on the context, before any bucket is defined): an archive of one
    // int8 parameter (the codes) and one uint8 buffer (the scales) is an owner's update against the reply it last
    // loaded, expanded on the GPU (fa_submit_mx8)
    bool mx8 = false;
    // --mx8-reply (implies --mx8): the buckets have the MX8 reply stage (fa_set_mx8_reply on the context); an owner
    // whose receipt of the round was an MX8 archive gets the new model back as one, its own archive the template
    bool mx8_reply = false;
    bool gpu_crc = true;  // --crc gpu|host: the reply records' CRC-32s from the GPU (fa_output_crc32) or the host
    std::map<int, double> samples;  // client id -> n_k
    // --server-opt RULE --server-lr L [--server-beta1 B] [--server-beta2 B] [--server-tau T]: the server
    // optimizer of every bucket (fa_set_server_opt on the context, before any bucket is defined);
    // --server-state FILE: read at startup if it exists, rewritten after every round
    fa_server_opt server{FA_OPT_NONE, 0.0f, 0.9f, 0.99f, 1e-3f};
    bool server_lr_given = false, server_flag = false;  // server_flag: some --server-* other than --server-opt
    std::string server_state;
    // --clip-norm C: the clip stage of every bucket (fa_set_clip on the context, before any bucket is defined);
    // --clip-state FILE: the buckets' references, read at startup if it exists, rewritten after every round
    float clip_norm = 0.0f;
    bool clip_given = false;
    std::string clip_state;
    // --krum-f F [--krum-m M]: the Krum stage of every bucket (fa_set_krum on the context, before any bucket is
    // defined); M defaults to DATA_OWNERS - F
    int krum_f = 0, krum_m = -1;
    bool krum_given = false, krum_m_given = false;
    // --geomed-iters T [--geomed-nu NU]: the geomed stage of every bucket (fa_set_geomed on the context, before any
    // bucket is defined); NU defaults to 1e-6
    int geomed_iters = 0;
    float geomed_nu = 1e-6f;
    bool geomed_given = false, geomed_nu_given = false;
    // --dp-noise-multiplier Z [--dp-seed S]: the noise stage of every bucket (fa_set_noise on the context, before any
    // bucket is defined) with stddev = Z * C * max_k w_k, C the --clip-norm; the seed comes from the operating
    // system's entropy at every start unless --dp-seed fixes it
    double dp_z = 0.0;
    uint64_t dp_seed = 0;
    bool dp_given = false, dp_seed_given = false;
};

const char* server_rule_name(int rule) {
    return rule == FA_OPT_MOMENTUM ? "momentum" : rule == FA_OPT_ADAGRAD ? "adagrad" : rule == FA_OPT_ADAM ? "adam" : "yogi";
}

// --server-state FILE, little-endian: "FASRVOPT", u32 version = 1, u32 rule, u32 n_parts, u32 0; then per part
// i32 part id (the protocol's model_part), u32 0, u64 n, u64 steps, x, m, v (n fp32 each; v zeros for
// momentum).  Hyperparameters are not stored: they come from the flags.
struct ServerStatePart {
    uint64_t n = 0, steps = 0;
    std::vector<float> x, m, v;
};
using ServerState = std::map<int, ServerStatePart>;
constexpr char kStateMagic[8] = {'F', 'A', 'S', 'R', 'V', 'O', 'P', 'T'};
constexpr uint32_t kStateVersion = 1;

// Reads FILE into *out.  A file that does not exist is an empty state (true); a bad magic, version, rule or a
// truncated file is an error (false, *err says which).
bool read_server_state(const std::string& path, int rule, ServerState* out, std::string* err) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return true;
    f.seekg(0, std::ios::end);
    const uint64_t size = (uint64_t)f.tellg();
    f.seekg(0);
    char magic[8];
    uint32_t hdr[4];
    if (!f.read(magic, 8) || !f.read(reinterpret_cast<char*>(hdr), 16)) return *err = "shorter than its header", false;
    if (std::memcmp(magic, kStateMagic, 8) != 0) return *err = "bad magic (not a FASRVOPT file)", false;
    if (hdr[0] != kStateVersion) return *err = "version " + std::to_string(hdr[0]) + ", expected 1", false;
    if ((int)hdr[1] != rule)
        return *err = "written with rule " + std::to_string(hdr[1]) + ", --server-opt " + server_rule_name(rule) +
                      " is rule " + std::to_string(rule), false;
    uint64_t at = 24;
    for (uint32_t i = 0; i < hdr[2]; ++i) {
        int32_t id[2];
        uint64_t ns[2];
        if (!f.read(reinterpret_cast<char*>(id), 8) || !f.read(reinterpret_cast<char*>(ns), 16))
            return *err = "truncated at part " + std::to_string(i), false;
        at += 24;
        if (ns[0] > (size - at) / 12) return *err = "part " + std::to_string(id[0]) + " runs past the end of the file", false;
        ServerStatePart& sp = (*out)[id[0]];
        sp.n = ns[0];
        sp.steps = ns[1];
        for (auto* a : {&sp.x, &sp.m, &sp.v}) {
            a->resize((size_t)sp.n);
            if (sp.n && !f.read(reinterpret_cast<char*>(a->data()), (std::streamsize)(sp.n * 4)))
                return *err = "truncated in part " + std::to_string(id[0]), false;
        }
        at += sp.n * 12;
    }
    return true;
}

// Writes FILE.tmp and renames it over FILE, so a reader never sees half a state.
bool write_server_state(const std::string& path, int rule, const ServerState& st) {
    const std::string tmp = path + ".tmp";
    {
        std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
        const uint32_t hdr[4] = {kStateVersion, (uint32_t)rule, (uint32_t)st.size(), 0};
        f.write(kStateMagic, 8);
        f.write(reinterpret_cast<const char*>(hdr), 16);
        for (auto& kv : st) {
            const int32_t id[2] = {kv.first, 0};
            const uint64_t ns[2] = {kv.second.n, kv.second.steps};
            f.write(reinterpret_cast<const char*>(id), 8);
            f.write(reinterpret_cast<const char*>(ns), 16);
            for (auto* a : {&kv.second.x, &kv.second.m, &kv.second.v})
                f.write(reinterpret_cast<const char*>(a->data()), (std::streamsize)(kv.second.n * 4));
        }
        f.flush();
        if (!f) return false;
    }
    return std::rename(tmp.c_str(), path.c_str()) == 0;
}

// --clip-state FILE, little-endian: "FACLIPRF", u32 version = 1, u32 n_parts; then per part i32 part id (the
// protocol's model_part), u32 0, u64 n, and the reference (n fp32).
using ClipState = std::map<int, std::vector<float>>;
constexpr char kClipMagic[8] = {'F', 'A', 'C', 'L', 'I', 'P', 'R', 'F'};

// Reads FILE into *out.  A file that does not exist is an empty state (true); a bad magic or version or a
// truncated file is an error (false, *err says which).
bool read_clip_state(const std::string& path, ClipState* out, std::string* err) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return true;
    f.seekg(0, std::ios::end);
    const uint64_t size = (uint64_t)f.tellg();
    f.seekg(0);
    char magic[8];
    uint32_t hdr[2];
    if (!f.read(magic, 8) || !f.read(reinterpret_cast<char*>(hdr), 8)) return *err = "shorter than its header", false;
    if (std::memcmp(magic, kClipMagic, 8) != 0) return *err = "bad magic (not a FACLIPRF file)", false;
    if (hdr[0] != 1) return *err = "version " + std::to_string(hdr[0]) + ", expected 1", false;
    uint64_t at = 16;
    for (uint32_t i = 0; i < hdr[1]; ++i) {
        int32_t id[2];
        uint64_t n;
        if (!f.read(reinterpret_cast<char*>(id), 8) || !f.read(reinterpret_cast<char*>(&n), 8))
            return *err = "truncated at part " + std::to_string(i), false;
        at += 16;
        if (n > (size - at) / 4) return *err = "part " + std::to_string(id[0]) + " runs past the end of the file", false;
        std::vector<float>& g = (*out)[id[0]];
        g.resize((size_t)n);
        if (n && !f.read(reinterpret_cast<char*>(g.data()), (std::streamsize)(n * 4)))
            return *err = "truncated in part " + std::to_string(id[0]), false;
        at += n * 4;
    }
    return true;
}

// Writes FILE.tmp and renames it over FILE, so a reader never sees half a state.
bool write_clip_state(const std::string& path, const ClipState& st) {
    const std::string tmp = path + ".tmp";
    {
        std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
        const uint32_t hdr[2] = {1, (uint32_t)st.size()};
        f.write(kClipMagic, 8);
        f.write(reinterpret_cast<const char*>(hdr), 8);
        for (auto& kv : st) {
            const int32_t id[2] = {kv.first, 0};
            const uint64_t n = kv.second.size();
            f.write(reinterpret_cast<const char*>(id), 8);
            f.write(reinterpret_cast<const char*>(&n), 8);
            f.write(reinterpret_cast<const char*>(kv.second.data()), (std::streamsize)(n * 4));
        }
        f.flush();
        if (!f) return false;
    }
    return std::rename(tmp.c_str(), path.c_str()) == 0;
}

void usage() {
    std::cerr << "usage: fa_aggregator -i ID -d DATA_OWNERS -c COMPUTE_NODES [--mode fedavg|literal|trimmed|median|bulyan]\n"
                 "       [--trim T] [--bulyan-f F] [--gpus G]\n"
                 "       [--rounds R] [--port-base P] [--discover] [--link-mbps M] [--samples id:n,...]\n"
                 "       [--divisor K] [--last-layers L] [--no-pinned] [--layout range|rs] [--rs-chunks C]\n"
                 "       [--eager] [--stall-report S] [--receipt-timeout S] [--rx-concurrency K]\n"
                 "       [--senders S] [--stream-min-bytes N] [--crc gpu|host] [--test-shared-device]\n"
                 "       [--server-opt momentum|adagrad|adam|yogi --server-lr L [--server-beta1 B] [--server-beta2 B]\n"
                 "        [--server-tau T] [--server-state FILE]]\n"
                 "       [--clip-norm C [--clip-state FILE]]\n"
                 "       [--krum-f F [--krum-m M]]\n"
                 "       [--geomed-iters T [--geomed-nu NU]]\n"
                 "       [--dp-noise-multiplier Z [--dp-seed S]]\n"
                 "       [--mx8] [--mx8-reply]\n"
                 "--mode trimmed: per element the T lowest and T highest of the owners' values are dropped and the\n"
                 "rest averaged (2T < DATA_OWNERS <= 128; without --trim, and with --mode median, the median), so up\n"
                 "to T owners that send NaN, inf or huge values change no reply; --samples is ignored; not with\n"
                 "--layout rs.\n"
                 "--mode bulyan --bulyan-f F: per bucket DATA_OWNERS - 2F owners are picked by running Krum repeatedly\n"
                 "over the owners' pairwise distances, then per element the picked values closest to their median are\n"
                 "averaged (all but 2F of them): F is the number of owners assumed Byzantine, 0 <= F, 4F + 3 <=\n"
                 "DATA_OWNERS <= 128; --samples is ignored; not with --trim, --clip-norm, --krum-f, --geomed-iters or\n"
                 "--layout rs.\n"
                 "--server-opt: a server optimizer (FedAvgM, FedAdagrad, FedAdam, FedYogi) steps the global model with\n"
                 "the round's aggregate; the model and its moments stay on the GPU in fp32; L finite and >= 0, B in\n"
                 "[0, 1) (defaults 0.9 and 0.99), T finite and > 0 (default 1e-3); --server-state FILE is read at startup\n"
                 "if it exists (the initial global model, the moments of an earlier run) and rewritten after every\n"
                 "round; not with --mode literal or --layout rs.\n"
                 "--clip-norm C: every owner's update (its receipt minus the global model it was last sent) is scaled\n"
                 "down to an L2 norm of at most C (finite and > 0) before the weighted average, and an owner whose\n"
                 "update holds a NaN or an inf is left out of the round; the first round of a bucket without a stored\n"
                 "model clips nothing; --clip-state FILE is read at startup if it exists (the model last sent) and\n"
                 "rewritten after every round; not with --mode literal|trimmed|median or --layout rs.\n"
                 "--krum-f F: per bucket only the M owners (--krum-m, default DATA_OWNERS - F; 1 is Krum) whose receipts\n"
                 "lie closest to the others' are averaged, with their own weights scaled up to the round's mass; F is\n"
                 "the number of owners assumed Byzantine, 0 <= F, 2F + 2 < DATA_OWNERS <= 128, 1 <= M <= DATA_OWNERS - F;\n"
                 "not with --clip-norm, --mode literal|trimmed|median or --layout rs.\n"
                 "--geomed-iters T: per bucket the owners' weighted geometric median instead of their weighted mean, by T\n"
                 "smoothed Weiszfeld passes (RFA): an owner is down-weighted by its distance from the running estimate,\n"
                 "with NU (--geomed-nu, default 1e-6, finite and > 0) as the floor on a distance; nobody is left out but\n"
                 "an owner that sends a NaN or an inf; 1 <= T <= 64, DATA_OWNERS <= 128; not with --clip-norm, --krum-f,\n"
                 "--mode literal|trimmed|median|bulyan or --layout rs.\n"
                 "--dp-noise-multiplier Z (with --clip-norm C): Gaussian noise of standard deviation Z * C * max_k w_k (w_k\n"
                 "the round's weights: the sensitivity of the clipped weighted sum to one owner) is added to every bucket's\n"
                 "aggregate before it is stepped or replied: DP-FedAvg.  The seed is drawn from the operating system at\n"
                 "every start, never stored, and no noise is ever replayed; --dp-seed S (u64) fixes it to reproduce a run,\n"
                 "which voids the guarantee.  Z finite and > 0; not with --mode literal or --layout rs.\n"
                 "--mx8: a receipt may be an MX8 archive -- one int8 parameter of n codes and one uint8 buffer of\n"
                 "ceil(n / 32) block scales -- holding the owner's update against the reply it last loaded, 33 bytes per 32\n"
                 "elements; it is expanded on the GPU and counts as that owner's receipt.  A bucket is still defined by its\n"
                 "first full receipt, which is also the reply's template, and needs one reduced round before it takes MX8\n"
                 "receipts (exit 1 otherwise); a round may mix both kinds; not with --mode literal or --layout rs.\n"
                 "--mx8-reply (implies --mx8): an owner whose receipt of the round was an MX8 archive gets the new model\n"
                 "back as one -- its own archive with the codes and scales of new model minus the model it was last sent,\n"
                 "which it adds to that model (decode rule 3); every other owner gets the full reply, which then holds\n"
                 "that same sum.  The round line reports mx8_replies, mx8_bytes_out and mx8_nan_blocks.\n"
                 "A bucket takes the dtype of its first receipt's parameters (all fp32, all bf16 or all fp16, by\n"
                 "their storage type) and is reduced and replied in it; a later receipt of another size or dtype\n"
                 "ends the process (exit 1).\n";
}

bool parse_args(int argc, char** argv, Options* o) {
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&](const char* what) -> const char* {
            if (i + 1 >= argc) {
                std::cerr << "missing value for " << what << "\n";
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "-i" || a == "--id") o->id = std::atoi(val("-i"));
        else if (a == "-d" || a == "--data_owners") o->data_owners = std::atoi(val("-d"));
        else if (a == "-c" || a == "--compute_nodes") o->compute_nodes = std::atoi(val("-c"));
        else if (a == "--gpus") o->gpus = std::atoi(val("--gpus"));
        else if (a == "--rounds") o->rounds = std::atoi(val("--rounds"));
        else if (a == "--port-base") o->port_base = std::atoi(val("--port-base"));
        else if (a == "--last-layers") o->last_layers = std::atoi(val("--last-layers"));
        else if (a == "--divisor") o->divisor = (float)std::atof(val("--divisor"));
        else if (a == "--discover") o->discover = true;
        else if (a == "--no-pinned") o->pinned = false;
        else if (a == "--eager") o->eager = true;
        else if (a == "--test-shared-device") o->shared_device = true;
        else if (a == "--mx8") o->mx8 = true;
        else if (a == "--mx8-reply") o->mx8 = o->mx8_reply = true;
        else if (a == "--rs-chunks") o->rs_chunks = std::atoi(val("--rs-chunks"));
        else if (a == "--stall-report") o->stall_report_s = std::atof(val("--stall-report"));
        else if (a == "--receipt-timeout") o->receipt_timeout_s = std::atof(val("--receipt-timeout"));
        else if (a == "--rx-concurrency") o->rx_concurrency = std::atoi(val("--rx-concurrency"));
        else if (a == "--senders") o->senders = std::atoi(val("--senders"));
        else if (a == "--stream-min-bytes") o->stream_min = (size_t)std::strtoull(val("--stream-min-bytes"), nullptr, 0);
        else if (a == "--crc") {
            std::string c = val("--crc");
            if (c == "host") o->gpu_crc = false;
            else if (c != "gpu") return false;
        }
        else if (a == "--layout") {
            std::string l = val("--layout");
            if (l == "rs") o->rs = true;
            else if (l != "range") return false;
        }
        else if (a == "--link-mbps") o->link_mbps = std::atof(val("--link-mbps"));
        else if (a == "--mode") {
            std::string m = val("--mode");
            if (m == "literal") o->mode = FA_LITERAL;
            else if (m == "fedavg") o->mode = FA_FEDAVG;
            else if (m == "trimmed") o->mode = FA_TRIMMED;
            else if (m == "median") o->mode = FA_TRIMMED, o->median = true;
            else if (m == "bulyan") o->mode = FA_TRIMMED, o->bulyan = true;
            else return false;
        } else if (a == "--server-opt") {
            std::string r = val("--server-opt");
            if (r == "momentum") o->server.rule = FA_OPT_MOMENTUM;
            else if (r == "adagrad") o->server.rule = FA_OPT_ADAGRAD;
            else if (r == "adam") o->server.rule = FA_OPT_ADAM;
            else if (r == "yogi") o->server.rule = FA_OPT_YOGI;
            else {
                std::cerr << "--server-opt " << r << ": momentum, adagrad, adam or yogi\n";
                return false;
            }
        } else if (a == "--server-lr") {
            o->server.lr = (float)std::atof(val("--server-lr"));
            o->server_lr_given = o->server_flag = true;
        } else if (a == "--server-beta1") {
            o->server.beta1 = (float)std::atof(val("--server-beta1"));
            o->server_flag = true;
        } else if (a == "--server-beta2") {
            o->server.beta2 = (float)std::atof(val("--server-beta2"));
            o->server_flag = true;
        } else if (a == "--server-tau") {
            o->server.tau = (float)std::atof(val("--server-tau"));
            o->server_flag = true;
        } else if (a == "--server-state") {
            o->server_state = val("--server-state");
            o->server_flag = true;
        } else if (a == "--clip-norm") {
            o->clip_norm = (float)std::atof(val("--clip-norm"));
            o->clip_given = true;
        } else if (a == "--clip-state") {
            o->clip_state = val("--clip-state");
        } else if (a == "--bulyan-f") {
            o->bulyan_f = std::atoi(val("--bulyan-f"));
            o->bulyan_f_given = true;
        } else if (a == "--krum-f") {
            o->krum_f = std::atoi(val("--krum-f"));
            o->krum_given = true;
        } else if (a == "--krum-m") {
            o->krum_m = std::atoi(val("--krum-m"));
            o->krum_m_given = true;
        } else if (a == "--geomed-iters") {
            o->geomed_iters = std::atoi(val("--geomed-iters"));
            o->geomed_given = true;
        } else if (a == "--geomed-nu") {
            o->geomed_nu = (float)std::atof(val("--geomed-nu"));
            o->geomed_nu_given = true;
        } else if (a == "--dp-noise-multiplier") {
            o->dp_z = std::atof(val("--dp-noise-multiplier"));
            o->dp_given = true;
        } else if (a == "--dp-seed") {
            o->dp_seed = (uint64_t)std::strtoull(val("--dp-seed"), nullptr, 0);
            o->dp_seed_given = true;
        } else if (a == "--trim") {
            o->trim = std::atoi(val("--trim"));
            o->trim_given = true;
        } else if (a == "--samples") {
            std::stringstream ss(val("--samples"));
            std::string tok;
            while (std::getline(ss, tok, ',')) {
                const size_t c = tok.find(':');
                if (c == std::string::npos) return false;
                o->samples[std::atoi(tok.substr(0, c).c_str())] = std::atof(tok.substr(c + 1).c_str());
            }
        } else if (a == "-h" || a == "--help") {
            return false;
        } else {
            std::cerr << "unknown argument " << a << "\n";
            return false;
        }
    }
    if (o->mx8 && (o->mode == FA_LITERAL || o->rs)) {
        std::cerr << (o->mx8_reply ? "--mx8-reply implies --mx8, which" : "--mx8")
                  << " expands an update against the bucket's last output on the GPU that holds it: not with "
                  << (o->rs ? "--layout rs" : "--mode literal") << "\n";
        return false;
    }
    if (o->trim_given && (o->mode != FA_TRIMMED || o->median || o->bulyan)) {
        std::cerr << "--trim goes with --mode trimmed\n";
        return false;
    }
    if (o->bulyan != o->bulyan_f_given) {
        std::cerr << "--mode bulyan and --bulyan-f F go together\n";
        return false;
    }
    if (o->bulyan) {
        if (o->rs) {
            std::cerr << "--mode bulyan needs every owner's bucket on one GPU: not with --layout rs\n";
            return false;
        }
        if (o->clip_given || o->krum_given) {
            std::cerr << "--mode bulyan selects and averages by itself: not with "
                      << (o->clip_given ? "--clip-norm" : "--krum-f") << "\n";
            return false;
        }
        if (o->bulyan_f < 0 || 4 * o->bulyan_f + 3 > o->data_owners || o->data_owners > FA_TRIMMED_MAX_CLIENTS) {
            std::cerr << "--bulyan-f " << o->bulyan_f << ": 0 <= F and 4F + 3 <= DATA_OWNERS <= " << FA_TRIMMED_MAX_CLIENTS
                      << ", got " << o->data_owners << " data owners\n";
            return false;
        }
    }
    if (o->mode == FA_TRIMMED) {
        if (o->rs) {
            std::cerr << "--mode trimmed|median needs every owner's value of an element on one GPU: not with --layout rs\n";
            return false;
        }
        if (o->data_owners > FA_TRIMMED_MAX_CLIENTS) {
            std::cerr << "--mode trimmed|median takes at most " << FA_TRIMMED_MAX_CLIENTS << " data owners\n";
            return false;
        }
        if (o->trim_given && (o->trim < 0 || 2 * o->trim >= o->data_owners)) {
            std::cerr << "--trim " << o->trim << ": 0 <= 2T < " << o->data_owners << " data owners\n";
            return false;
        }
        if (!o->trim_given) o->trim = o->data_owners >= 1 ? (o->data_owners - 1) / 2 : 0;
    }
    if (o->server.rule == FA_OPT_NONE && o->server_flag) {
        std::cerr << "--server-lr, --server-beta1, --server-beta2, --server-tau and --server-state go with --server-opt\n";
        return false;
    }
    if (o->server.rule != FA_OPT_NONE) {
        const fa_server_opt& so = o->server;
        const bool adaptive = so.rule != FA_OPT_MOMENTUM, second = so.rule == FA_OPT_ADAM || so.rule == FA_OPT_YOGI;
        if (!o->server_lr_given) {
            std::cerr << "--server-opt needs --server-lr\n";
            return false;
        }
        if (o->mode == FA_LITERAL) {
            std::cerr << "--server-opt steps a mean: not with --mode literal\n";
            return false;
        }
        if (o->rs) {
            std::cerr << "--server-opt needs a bit-specified aggregate: not with --layout rs\n";
            return false;
        }
        if (!std::isfinite(so.lr) || so.lr < 0) {
            std::cerr << "--server-lr " << so.lr << ": finite and >= 0\n";
            return false;
        }
        if (!(so.beta1 >= 0 && so.beta1 < 1)) {
            std::cerr << "--server-beta1 " << so.beta1 << ": in [0, 1)\n";
            return false;
        }
        if (second && !(so.beta2 >= 0 && so.beta2 < 1)) {
            std::cerr << "--server-beta2 " << so.beta2 << ": in [0, 1)\n";
            return false;
        }
        if (adaptive && (!std::isfinite(so.tau) || !(so.tau > 0))) {
            std::cerr << "--server-tau " << so.tau << ": finite and > 0\n";
            return false;
        }
    }
    if (!o->dp_given && o->dp_seed_given) {
        std::cerr << "--dp-seed goes with --dp-noise-multiplier\n";
        return false;
    }
    if (o->dp_given) {
        if (o->mode == FA_LITERAL) {
            std::cerr << "--dp-noise-multiplier adds noise to a clipped weighted average: not with --mode literal\n";
            return false;
        }
        if (o->rs) {
            std::cerr << "--dp-noise-multiplier needs a bit-specified aggregate: not with --layout rs\n";
            return false;
        }
        if (!o->clip_given) {
            std::cerr << "--dp-noise-multiplier needs --clip-norm C: the noise is scaled to the clipped sum's sensitivity\n";
            return false;
        }
        if (!std::isfinite(o->dp_z) || !(o->dp_z > 0)) {
            std::cerr << "--dp-noise-multiplier " << o->dp_z << ": finite and > 0\n";
            return false;
        }
    }
    if (!o->clip_given && !o->clip_state.empty()) {
        std::cerr << "--clip-state goes with --clip-norm\n";
        return false;
    }
    if (o->clip_given) {
        if (o->mode != FA_FEDAVG) {
            std::cerr << "--clip-norm clips the updates of a weighted average: not with --mode "
                      << (o->mode == FA_LITERAL ? "literal" : o->median ? "median" : "trimmed") << "\n";
            return false;
        }
        if (o->rs) {
            std::cerr << "--clip-norm needs a bit-specified aggregate: not with --layout rs\n";
            return false;
        }
        if (!std::isfinite(o->clip_norm) || !(o->clip_norm > 0)) {
            std::cerr << "--clip-norm " << o->clip_norm << ": finite and > 0\n";
            return false;
        }
    }
    if (!o->krum_given && o->krum_m_given) {
        std::cerr << "--krum-m goes with --krum-f\n";
        return false;
    }
    if (o->krum_given) {
        if (o->clip_given) {
            std::cerr << "--krum-f and --clip-norm do not compose: one of them\n";
            return false;
        }
        if (o->mode != FA_FEDAVG) {
            std::cerr << "--krum-f selects the owners of a weighted average: not with --mode "
                      << (o->mode == FA_LITERAL ? "literal" : o->median ? "median" : "trimmed") << "\n";
            return false;
        }
        if (o->rs) {
            std::cerr << "--krum-f needs both owners of a pair on one GPU: not with --layout rs\n";
            return false;
        }
        if (o->data_owners > FA_KRUM_MAX_CLIENTS) {
            std::cerr << "--krum-f takes at most " << FA_KRUM_MAX_CLIENTS << " data owners\n";
            return false;
        }
        if (o->krum_f < 0 || 2 * o->krum_f + 2 >= o->data_owners) {
            std::cerr << "--krum-f " << o->krum_f << ": 0 <= F and 2F + 2 < " << o->data_owners << " data owners\n";
            return false;
        }
        if (!o->krum_m_given) o->krum_m = o->data_owners - o->krum_f;
        if (o->krum_m < 1 || o->krum_m > o->data_owners - o->krum_f) {
            std::cerr << "--krum-m " << o->krum_m << ": 1 <= M <= " << o->data_owners - o->krum_f
                      << " (DATA_OWNERS - F)\n";
            return false;
        }
    }
    if (!o->geomed_given && o->geomed_nu_given) {
        std::cerr << "--geomed-nu goes with --geomed-iters\n";
        return false;
    }
    if (o->geomed_given) {
        if (o->clip_given || o->krum_given) {
            std::cerr << "--geomed-iters and " << (o->clip_given ? "--clip-norm" : "--krum-f") << " do not compose: one of them\n";
            return false;
        }
        if (o->mode != FA_FEDAVG) {
            std::cerr << "--geomed-iters re-weights the owners of a weighted average: not with --mode "
                      << (o->mode == FA_LITERAL ? "literal" : o->bulyan ? "bulyan" : o->median ? "median" : "trimmed") << "\n";
            return false;
        }
        if (o->rs) {
            std::cerr << "--geomed-iters needs every owner's value of an element on one GPU: not with --layout rs\n";
            return false;
        }
        if (o->data_owners > FA_GEOMED_MAX_CLIENTS) {
            std::cerr << "--geomed-iters takes at most " << FA_GEOMED_MAX_CLIENTS << " data owners\n";
            return false;
        }
        if (o->geomed_iters < 1 || o->geomed_iters > FA_GEOMED_MAX_ITERS) {
            std::cerr << "--geomed-iters " << o->geomed_iters << ": 1 <= T <= " << FA_GEOMED_MAX_ITERS << "\n";
            return false;
        }
        if (!std::isfinite(o->geomed_nu) || !(o->geomed_nu > 0)) {
            std::cerr << "--geomed-nu " << o->geomed_nu << ": finite and > 0\n";
            return false;
        }
    }
    return o->data_owners >= 1 && o->stall_report_s > 0 && o->receipt_timeout_s >= 0;
}

// parts[1].layers.size() for the aggregator's ModelPart(start, -1) (systemAPI.cpp:19):
// resnet_part / lenet_part always return two Sequentials for end == -1
// (resnet_split.cpp:176-188, lenet_help.cpp:170-183); vgg_part returns two iff
// start - 1 <= 20 (vgg_help.cpp:250-256, ModelPart passes start - 1, models.h:25).
int last_part_layers(int model_name, int start) {
    if (model_name == 0) return (start - 1) <= 20 ? 2 : 1;
    return 2;
}

long now_ms() {
    return std::chrono::duration_cast<std::chrono::milliseconds>(
               std::chrono::system_clock::now().time_since_epoch())
        .count();
}

double secs_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

#define FA_CHECK(call)                                                                       \
    do {                                                                                     \
        int rc_ = (call);                                                                    \
        if (rc_ != FA_OK) {                                                                  \
            std::cerr << "[aggregator] " #call " failed: " << fa_last_error() << "\n";       \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

// Replies of at least this many parameter bytes get their records' CRC-32s from the GPU (fa_output_crc32);
// smaller ones are sealed on the host, which takes less than the call's round trip.
constexpr size_t kGpuCrcMinBytes = 1u << 20;

class Aggregator {
public:
    Aggregator(const Options& o, NetLayer* net, const std::vector<int>& owners, ServerState loaded, ClipState clip_loaded)
        : o_(o), net_(net), loaded_(std::move(loaded)), clip_loaded_(std::move(clip_loaded)) {
        int flags = o.rs ? FA_SHARD_CLIENT_RS : o.gpus > 1 ? FA_SHARD_RANGE : 0;
        if (o.eager) flags |= FA_ACCUMULATE_ON_ARRIVAL;
        if (o.shared_device) {
            const std::vector<int> zeros((size_t)std::max(1, o.gpus), 0);
            FA_CHECK(fa_create_ex(&ctx_, zeros.data(), o.gpus, flags | FA_TEST_SHARED_DEVICE));
        } else {
            FA_CHECK(fa_create(&ctx_, o.gpus, flags));
        }
        FA_CHECK(fa_set_literal_divisor(ctx_, -1, o.divisor));
        if (o.mode == FA_TRIMMED) FA_CHECK(fa_set_trim(ctx_, -1, o.trim));
        if (o.bulyan) FA_CHECK(fa_set_bulyan(ctx_, -1, o.bulyan_f));  // before any bucket
        if (o.server.rule != FA_OPT_NONE) FA_CHECK(fa_set_server_opt(ctx_, -1, &o.server));  // before any bucket
        if (o.clip_given) FA_CHECK(fa_set_clip(ctx_, -1, o.clip_norm));
        if (o.krum_given) FA_CHECK(fa_set_krum(ctx_, -1, o.krum_f, o.krum_m));
        if (o.geomed_given) FA_CHECK(fa_set_geomed(ctx_, -1, o.geomed_iters, o.geomed_nu));
        if (o.mx8) FA_CHECK(fa_set_mx8(ctx_, -1, 1));  // before any bucket
        if (o.mx8_reply) FA_CHECK(fa_set_mx8_reply(ctx_, -1, 1));
        if (o.rs_chunks > 0) {
            fa_tuning t{};
            t.rs_chunks = o.rs_chunks;
            FA_CHECK(fa_ctx_set_tuning(ctx_, &t));
        }
        std::vector<int> order = owners;
        if ((int)order.size() != o.data_owners) {
            order = {0};
            for (int i = 0; i < o.data_owners - 1; ++i) order.push_back(i + o.compute_nodes + 1);
        }
        for (int k = 0; k < (int)order.size(); ++k) slots_.insert({order[k], k});
        expected_ = order;
        if (o.dp_given) {  // before any bucket: stddev = Z C max_k w_k, the add/remove sensitivity of the clipped sum
            float wmax = 0.0f;
            for (int id : expected_) wmax = std::max(wmax, weight_of(id));
            dp_stddev_ = (float)(o.dp_z * (double)o.clip_norm * (double)wmax);
            if (!std::isfinite(dp_stddev_) || !(dp_stddev_ > 0)) {
                std::cerr << "[aggregator] --dp-noise-multiplier: Z * C * max weight = " << dp_stddev_ << " is not a usable stddev\n";
                std::exit(2);
            }
            uint64_t seed = o.dp_seed;
            if (o.dp_seed_given) {
                std::cerr << "[aggregator] DP NOISE: the seed is FIXED by --dp-seed: this run can be reproduced and its noise "
                             "is not private\n";
            } else {
                std::random_device rd;  // the operating system's entropy; nothing is persisted
                seed = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
            }
            FA_CHECK(fa_set_noise(ctx_, -1, dp_stddev_, seed));
        }
        claimed_.assign(o.data_owners, 0);
    }
    ~Aggregator() { fa_destroy(ctx_); }

    // Stale receipts across rounds (host/receipts.h): a byte copy of a receipt its owner already had reduced
    // (a late copy of an earlier round's) is dropped -- never counted, never in a slot.
    void end_phase() {
        ledger_.end_phase();
        // frames that ended without a receipt for this phase (a malformed frame, one still queued for the
        // next phase) need no stream any more: their receipts, if any, take the plain path
        streams_.erase(std::remove_if(streams_.begin(), streams_.end(),
                                      [](const Stream& s) { return s.in->ended.load(std::memory_order_acquire); }),
                       streams_.end());
    }

    // ---------------------------------------------------------------- streaming ingest
    //
    // The reference reads a whole frame before anything else happens (network_layer.cpp:48-65) and only then
    // decodes it (aggregator.cpp:63-64); so did this process until round 6, and a phase ended with the H2D
    // copies of the receipts that landed last.  The archive's parameter records (data/<key>) come first in
    // the zip, stored and 64-byte aligned, and every receipt of a bucket is the same module saved again: so
    // the records' places in a frame of a given length are those of the bucket's previous receipt.  A large
    // frame is announced while it arrives (NetLayer::set_streaming); once its owner and bucket are known and
    // the bucket has a layout for its length, each record is DMA'd to the slot as soon as its bytes are in
    // (fa_submit_piece_pinned).  When the frame is complete the archive is parsed as before; if its records
    // are where they were predicted, the slot is committed (fa_submit_commit), else the receipt is submitted
    // the plain way over the streamed bytes.  Only a slot whose owner has no receipt of the bucket yet this
    // phase is streamed into, by one frame at a time, and a receipt that lands whole stops any other frame
    // streaming into its slot -- so a stale copy can never overwrite a receipt taken (the ledger still judges
    // every frame once it is complete; a stream it drops was never committed).
    void set_phase(const std::vector<int>& mps) { phase_mps_ = std::set<int>(mps.begin(), mps.end()); }

    void pump() {
        intake();
        for (auto it = streams_.begin(); it != streams_.end();) {
            Stream& s = *it;
            if (s.in->failed.load(std::memory_order_acquire)) {  // the connection broke: nothing comes of it
                it = streams_.erase(it);
                continue;
            }
            if (s.slot < 0 && !s.cancelled) claim(s);
            if (s.slot >= 0) feed(s, s.in->have.load(std::memory_order_acquire));
            ++it;
        }
    }

    unsigned long long streamed() const { return streamed_; }
    unsigned long long stream_fallbacks() const { return stream_fallbacks_; }
    unsigned long long streamed_bytes() const { return streamed_bytes_; }

    static ReceiptKey key_of(const Receipt& r) {
        return ReceiptKey{r.t_start, r.blob_len, archive_fingerprint(r.blob(), r.blob_len)};
    }

    // A receipt of the other phase is never taken (see main): counted as a stale copy when it is a byte copy
    // of one already reduced, else as ignored (a retransmission of this round's).
    void other_phase(const Receipt& r, int phase) {
        take_stream(r);
        if (ledger_.is_reduced_copy(r.client_id, r.model_part, key_of(r))) {
            std::cerr << "[aggregator] stale part " << r.model_part << " from owner " << r.client_id
                      << " during phase " << phase << " (a byte copy of a receipt already reduced): dropped\n";
            ++stale_dropped_;
        } else {
            std::cerr << "[aggregator] part " << r.model_part << " from owner " << r.client_id << " during phase "
                      << phase << " (a retransmission of this round's): ignored\n";
            ++ignored_;
        }
    }

    // Consumes one receipt of bucket `mp` into its client slot.  Returns whether it is the first receipt of
    // this (owner, bucket) in the round: a retransmission replaces the slot's contents (the newest one wins,
    // as a second torch::load would) but is not another receipt -- the phase waits for D distinct owners.
    // A stale receipt (above) is dropped: returns false without touching the slot.
    bool absorb(const Receipt& r) {
        const Stream st = take_stream(r);  // the frame's own stream, if it was streamed into a slot
        const ReceiptKey key = key_of(r);
        const ReceiptLedger::Verdict v = ledger_.check(r.client_id, r.model_part, key);
        if (v.stale) {
            std::cerr << "[aggregator] stale part " << r.model_part << " from owner " << r.client_id << " (" << v.why
                      << "): dropped\n";
            ++stale_dropped_;
            return false;
        }
        if (!v.note.empty()) {
            std::cerr << "[aggregator] part " << r.model_part << " from owner " << r.client_id << " " << v.note << "\n";
            ++clock_back_;
        }
        const auto t0 = std::chrono::steady_clock::now();
        TorchArchive ar;
        std::string err;
        if (!ar.parse(r.blob(), r.blob_len, &err)) {
            std::cerr << "[aggregator] receipt from " << r.client_id << ": " << err << "\n";
            std::exit(1);
        }
        Bucket& b = buckets_[r.model_part];
        const int8_t* mq = nullptr;
        const uint8_t* me = nullptr;
        int64_t mn = 0;
        if (o_.mx8 && ar.mx8_view(&mq, &me, &mn)) return absorb_mx8(r, st.slot >= 0, key, mq, me, mn, t0);
        // the bucket dtype, from the parameters' storage type (never from the element size: bf16 and fp16
        // are both 2 bytes): fp32 (the reference), bf16 (config C3) or fp16 (owners that train with .half())
        const ParamDtype pd = ar.param_dtype();
        const int es = ar.param_elem_size();
        if (!b.defined) {
            if (pd == ParamDtype::None) {
                std::cerr << "[aggregator] bucket " << r.model_part << ": parameters not all fp32, bf16 or fp16\n";
                std::exit(1);
            }
            b.numel = (size_t)ar.param_numel();
            b.elem = es;
            b.dtype = pd;
            const fa_dtype dt = pd == ParamDtype::F32 ? FA_F32 : pd == ParamDtype::BF16 ? FA_BF16 : FA_F16;
            FA_CHECK(fa_bucket_define(ctx_, r.model_part, b.numel, dt, dt, o_.data_owners, o_.mode));
            b.defined = true;
            auto ls = loaded_.find(r.model_part);
            if (ls != loaded_.end()) {  // --server-state: the bucket starts from the stored model and moments
                const ServerStatePart& sp = ls->second;
                if (sp.n != b.numel) {
                    std::cerr << "[aggregator] --server-state: part " << r.model_part << " holds " << sp.n
                              << " elements, its bucket " << b.numel << "\n";
                    // the owners are still sending this phase's other receipts: the readers take their frame
                    // buffers from the process-wide allocator, which exit() destroys -- they finish first
                    net_->stop();
                    std::exit(1);
                }
                FA_CHECK(fa_server_opt_set_state(ctx_, r.model_part, sp.x.data(), sp.m.data(),
                                                 o_.server.rule == FA_OPT_MOMENTUM ? nullptr : sp.v.data(), sp.steps));
            }
            auto lc = clip_loaded_.find(r.model_part);
            if (lc != clip_loaded_.end()) {  // --clip-state: the model this bucket's owners were last sent
                if (lc->second.size() != b.numel) {
                    std::cerr << "[aggregator] --clip-state: part " << r.model_part << " holds " << lc->second.size()
                              << " elements, its bucket " << b.numel << "\n";
                    net_->stop();  // as for --server-state above
                    std::exit(1);
                }
                FA_CHECK(fa_clip_set_reference(ctx_, r.model_part, lc->second.data()));
            }
        } else if ((size_t)ar.param_numel() != b.numel || pd != b.dtype) {
            std::cerr << "[aggregator] bucket " << r.model_part << " changed size or dtype\n";
            std::exit(1);
        }
        const int slot = slot_of(r.client_id);
        cancel_streams(r.client_id, r.model_part);  // nothing else writes this slot from here on
        std::vector<const void*> ptrs;
        std::vector<size_t> bytes;
        if (ar.param_segments(&ptrs, &bytes)) {
            auto recs = records_of(r, ptrs, bytes);
            if (st.slot == slot && st.recs && *st.recs == *recs) {
                // streamed: the layout held; the records not sent yet go now, then the slot counts
                Stream done = st;
                feed(done, r.frame->size());
                FA_CHECK(fa_submit_commit(ctx_, r.model_part, slot, weight_of(r.client_id)));
                ++streamed_;
            } else if (r.frame->pinned) {  // DMA from the frame itself; it is held until the bucket is finalized
                if (st.slot >= 0) ++stream_fallbacks_;  // the layout changed: the plain submit overwrites
                FA_CHECK(fa_submit_gather_pinned(ctx_, r.model_part, slot, (int)ptrs.size(), ptrs.data(),
                                                 bytes.data(), weight_of(r.client_id)));
                b.held.push_back(r.frame);
            } else {
                FA_CHECK(fa_submit_gather(ctx_, r.model_part, slot, (int)ptrs.size(), ptrs.data(), bytes.data(),
                                          weight_of(r.client_id)));
            }
        } else {  // strided parameters: flatten first
            std::vector<uint8_t> flat(b.numel * (size_t)b.elem);
            if (!ar.gather_param_bytes(flat.data(), &err)) {
                std::cerr << "[aggregator] " << err << "\n";
                std::exit(1);
            }
            FA_CHECK(fa_submit(ctx_, r.model_part, slot, flat.data(), weight_of(r.client_id)));
        }
        if (r.frame->pinned && !ptrs.empty()) {  // the layout later frames of this length are streamed with
            b.recs = records_of(r, ptrs, bytes);
            b.recs_len = r.blob_len;
        }
        b.bytes_in += r.blob_len;
        ledger_.accept(r.client_id, r.model_part, key);
        const bool first = b.arrived.insert(r.client_id).second;
        b.last = r;  // template of the reply: the last full receipt (its buffers travel back, as in the reference)
        b.mx8_from.erase(r.client_id);  // a full receipt after an MX8 one of the same round: a full reply
        st_.absorb_s += secs_since(t0);
        if (!first) {
            std::cerr << "[aggregator] part " << r.model_part << ": owner " << r.client_id << " sent it again\n";
            ++replaced_;
        }
        return first;
    }

    // --mx8: an MX8 receipt (TorchArchive::mx8_view) of a defined bucket with a round behind it goes to its slot
    // as codes and scales -- DMA'd from the frame when that is pinned -- and is expanded there against the bucket's
    // last output.  Its frame was never streamed by the bucket's layout (claim() matches a frame's length against
    // the last full receipt's; should the two ever agree, the expansion overwrites the whole slot).  It is not the
    // reply's template: that stays the bucket's last full receipt.
    bool absorb_mx8(const Receipt& r, bool streamed, const ReceiptKey& key, const int8_t* q, const uint8_t* e, int64_t n,
                    std::chrono::steady_clock::time_point t0) {
        auto& b = buckets_[r.model_part];
        const char* why = !b.defined ? "is not defined yet (its first receipt must be a full one)"
                          : !b.reduced ? "has no round reduced yet (the update has nothing to be applied to)"
                          : (size_t)n != b.numel ? "holds another number of elements" : nullptr;
        if (why) {
            std::cerr << "[aggregator] MX8 receipt for part " << r.model_part << " from owner " << r.client_id
                      << ": the bucket " << why << "\n";
            net_->stop();  // as for --server-state: the readers finish before exit() destroys their allocator
            std::exit(1);
        }
        const int slot = slot_of(r.client_id);
        cancel_streams(r.client_id, r.model_part);
        if (streamed) ++stream_fallbacks_;
        FA_CHECK(fa_submit_mx8(ctx_, r.model_part, slot, q, e, weight_of(r.client_id), r.frame->pinned ? FA_HOST_PINNED : 0));
        if (r.frame->pinned) b.held.push_back(r.frame);  // DMA'd from until the bucket is finalized
        b.bytes_in += r.blob_len;
        ++mx8_receipts_;
        mx8_bytes_ += r.blob_len;
        if (o_.mx8_reply) b.mx8_from[r.client_id] = r;  // the template of this owner's reply
        ledger_.accept(r.client_id, r.model_part, key);
        const bool first = b.arrived.insert(r.client_id).second;
        st_.absorb_s += secs_since(t0);
        if (!first) {
            std::cerr << "[aggregator] part " << r.model_part << ": owner " << r.client_id << " sent it again\n";
            ++replaced_;
        }
        return first;
    }
    // This round's MX8 receipts and their archive bytes so far; reading them starts the next round's count.
    std::pair<unsigned long long, unsigned long long> take_mx8() {
        const auto v = std::make_pair(mx8_receipts_, mx8_bytes_);
        mx8_receipts_ = mx8_bytes_ = 0;
        return v;
    }
    // This round's MX8 replies, their archive bytes and the E = 255 blocks of its codes; reading them starts the next
    // round's count.
    struct Mx8Out {
        unsigned long long replies, bytes, nan_blocks;
    };
    Mx8Out take_mx8_out() {
        const Mx8Out v{mx8_replies_, mx8_bytes_out_, mx8_nan_blocks_};
        mx8_replies_ = mx8_bytes_out_ = mx8_nan_blocks_ = 0;
        return v;
    }

    // The replies of one bucket: the full one (null when every owner gets its own) and, by owner id, the MX8 ones.
    struct Replies {
        std::shared_ptr<const Bytes> full;
        std::map<int, std::shared_ptr<const Bytes>> mx8;
    };
    std::vector<int> destinations() const {  // node 0 and the data owners i + c + 1, i < D - 1
        std::vector<int> ids = {0};
        for (int i = 0; i < o_.data_owners - 1; ++i) ids.push_back(i + o_.compute_nodes + 1);
        return ids;
    }

    // --mx8-reply: the MX8 replies of bucket mp for the owners whose receipt of this round was an MX8 archive, each
    // the owner's own archive with the round's codes and scales in its two records (TorchArchive::with_mx8_into).
    // The codes come from fa_finalize_mx8, which ends the round, when nobody needs the full reply, else from
    // fa_copy_mx8 after the full reply ended it.
    void mx8_replies(int mp, bool round_open, Replies* out) {
        auto& b = buckets_[mp];
        std::vector<int8_t> q(b.numel);
        std::vector<uint8_t> e(fa_mx8_scale_bytes(b.numel));
        FA_CHECK(round_open ? fa_finalize_mx8(ctx_, mp, q.data(), e.data(), 0) : fa_copy_mx8(ctx_, mp, q.data(), e.data(), 0));
        for (auto& kv : b.mx8_from) {
            const Receipt& r = kv.second;
            TorchArchive ar;
            std::string err;
            Message m;
            m.type = OPERATION;
            m.client_id = o_.id;
            m.prev_node = o_.id;
            m.type_op = AGGREGATION;
            m.model_part = mp;
            m.t_start = now_ms();
            char* values = nullptr;
            std::shared_ptr<Bytes> f;
            if (ar.parse(r.blob(), r.blob_len, &err)) f = operation_frame(m, ar.size(), &values);
            if (!f || !ar.with_mx8_into(q.data(), e.data(), (int64_t)b.numel, (uint8_t*)values, &err)) {
                std::cerr << "[aggregator] MX8 reply for part " << mp << " to owner " << kv.first << ": " << err << "\n";
                std::exit(1);
            }
            out->mx8[kv.first] = f;
            ++mx8_replies_;
            mx8_bytes_out_ += ar.size();
        }
    }

    // Reduces bucket mp and returns the framed reply, built once and shared by every destination:
    // the last receipt's archive around the reduced parameters, which the D2H copy writes straight
    // into the frame's parameter records.
    Replies reduce(int mp) {
        Bucket& b = buckets_[mp];
        const auto t0 = std::chrono::steady_clock::now();
        Replies out;
        // owners without an MX8 receipt this round get the full reply; with none of them its D2H is skipped
        bool need_full = b.mx8_from.empty();
        for (int id : destinations()) need_full = need_full || !b.mx8_from.count(id);
        if (!need_full) {
            const auto t1 = std::chrono::steady_clock::now();
            mx8_replies(mp, true, &out);
            round_stats(mp);
            end_round(mp);
            st_.finalize_s += secs_since(t1);
            return out;
        }
        TorchArchive ar;
        std::string err;
        if (!ar.parse(b.last.blob(), b.last.blob_len, &err)) {
            std::cerr << "[aggregator] reply for part " << mp << ": " << err << "\n";
            std::exit(1);
        }
        Message m;  // Task(myid, aggregation_, myid) with model_part, aggregator.cpp:96-101
        m.type = OPERATION;
        m.client_id = o_.id;
        m.prev_node = o_.id;
        m.type_op = AGGREGATION;
        m.model_part = mp;
        m.t_start = now_ms();
        char* values = nullptr;
        auto f = operation_frame(m, ar.size(), &values);
        std::vector<void*> dsts;
        std::vector<size_t> bytes;
        double t_fin;
        if (ar.layout_into((uint8_t*)values, &dsts, &bytes, nullptr)) {
            const auto t1 = std::chrono::steady_clock::now();
            FA_CHECK(fa_finalize_gather(ctx_, mp, (int)dsts.size(), dsts.data(), bytes.data(),
                                        f->pinned ? FA_HOST_PINNED : 0));
            // the records' CRC-32s from the reduced bucket on the GPU (a few us; the host would read the
            // whole reply back); a part read in place into its reply has no device output: the host seals it
            std::vector<uint32_t> crcs(dsts.size());
            const bool gpu_crc = o_.gpu_crc && !bytes.empty() && b.numel * (size_t)b.elem >= kGpuCrcMinBytes &&
                                 fa_output_crc32(ctx_, mp, (int)bytes.size(), bytes.data(), crcs.data()) == FA_OK;
            t_fin = secs_since(t1);
            if (!gpu_crc || !ar.seal_params_with((uint8_t*)values, crcs.data())) ar.seal_params((uint8_t*)values);
        } else {  // strided parameters: through a flat copy
            const auto t1 = std::chrono::steady_clock::now();
            std::vector<uint8_t> out(b.numel * (size_t)b.elem);
            FA_CHECK(fa_finalize(ctx_, mp, out.data()));
            t_fin = secs_since(t1);
            if (!ar.with_param_bytes_into(out.data(), (uint8_t*)values, &err)) {
                std::cerr << "[aggregator] reply for part " << mp << ": " << err << "\n";
                std::exit(1);
            }
        }
        if (!b.mx8_from.empty()) mx8_replies(mp, false, &out);
        round_stats(mp);
        end_round(mp);
        st_.finalize_s += t_fin;
        st_.frame_s += secs_since(t0) - t_fin;
        out.full = f;
        return out;
    }

    void end_round(int mp) {
        auto& b = buckets_[mp];
        b.held.clear();
        b.arrived.clear();
        b.mx8_from.clear();
        b.bytes_in = 0;
        b.reduced = true;
    }

    // What the stages made of bucket mp's receipts in the reducing call just made, for the round line.
    void round_stats(int mp) {
        if (o_.mx8_reply) {
            uint64_t nan = 0;
            FA_CHECK(fa_mx8_reply_stats(ctx_, mp, &nan));
            mx8_nan_blocks_ += nan;
            if (nan)
                std::cerr << "[aggregator] MX8 REPLY: part " << mp << ": " << nan << " blocks of the new model are NaN (a "
                          << "NaN or an inf in the aggregate or in the model last sent); they stay NaN until the "
                          << "aggregator is restarted\n";
        }
        if (o_.clip_given) {  // what the clip stage did to this bucket's receipts, for the round line
            std::vector<double>& q = clip_q_[mp];
            q.assign((size_t)o_.data_owners, 0.0);
            std::vector<int> inc((size_t)o_.data_owners, 1);
            int clipped = 0;
            FA_CHECK(fa_clip_get_round(ctx_, mp, q.data(), nullptr, inc.data(), &clipped));
            clip_clipped_ += (unsigned long long)clipped;
            for (int i : inc) clip_excluded_ += i ? 0 : 1;
        }
        if (o_.krum_given) {  // what the Krum stage made of this bucket's receipts, for the round line
            KrumRound& kr = krum_[mp];
            kr.scores.assign((size_t)o_.data_owners, 0.0);
            kr.selected.assign((size_t)o_.data_owners, 0);
            int kept = 0;
            FA_CHECK(fa_krum_get_round(ctx_, mp, nullptr, kr.scores.data(), kr.selected.data(), &kept));
            if (kept == 0)
                std::cerr << "[aggregator] KRUM: part " << mp << ": NO OWNER SELECTED (every score is infinite): the "
                          << "reply of this bucket is all zeros\n";
        }
        if (o_.geomed_given) {  // what the geomed stage made of this bucket's receipts, for the round line
            const size_t D = (size_t)o_.data_owners;
            GeomedRound& gr = geomed_[mp];
            std::vector<double> q((size_t)FA_GEOMED_MAX_ITERS * D, 0.0);
            std::vector<float> w((size_t)(FA_GEOMED_MAX_ITERS + 1) * D, 0.0f);
            gr.included.assign(D, 0);
            FA_CHECK(fa_geomed_get_round(ctx_, mp, &gr.passes, q.data(), w.data(), gr.included.data(), nullptr));
            const size_t last = gr.passes > 0 ? (size_t)gr.passes - 1 : 0;
            gr.sumsq.assign(q.begin() + (ptrdiff_t)(last * D), q.begin() + (ptrdiff_t)((last + 1) * D));
            gr.weights.assign(w.begin() + (ptrdiff_t)((size_t)gr.passes * D), w.begin() + (ptrdiff_t)(((size_t)gr.passes + 1) * D));
            if (std::find(gr.included.begin(), gr.included.end(), 1) == gr.included.end())
                std::cerr << "[aggregator] GEOMED: part " << mp << ": NO OWNER LEFT (every weight is zero or every "
                          << "receipt holds a NaN or an inf): the reply of this bucket is all zeros\n";
        }
        if (o_.bulyan) {  // whom the Bulyan stage picked for this bucket, for the round line
            std::vector<int>& sel = bulyan_[mp];
            sel.assign((size_t)o_.data_owners, 0);
            int kept = 0;
            FA_CHECK(fa_bulyan_get_round(ctx_, mp, nullptr, nullptr, nullptr, sel.data(), &kept));
            if (kept == 0)
                std::cerr << "[aggregator] BULYAN: part " << mp << ": NO OWNER PICKED (every score is infinite): the "
                          << "reply of this bucket is all zeros\n";
        }
    }

    // Fan-out to node 0 and the data owners i + c + 1, i < D - 1 (aggregator.cpp:102-106, :158-164).
    void fan_out(const Replies& r) {
        for (int id : destinations()) {
            auto it = r.mx8.find(id);
            net_->send(id, it != r.mx8.end() ? it->second : r.full);
        }
    }

    // --server-state: every defined bucket's x, m, v and steps (parts read at startup and never defined in this
    // run are carried over as read), written to FILE.tmp and renamed over FILE.  Returns the most steps a
    // bucket has taken (the round line's server_steps).
    unsigned long long save_server_state() {
        unsigned long long most = 0;
        const bool write = !o_.server_state.empty();
        for (auto& kv : buckets_) {
            if (!kv.second.defined) continue;
            uint64_t steps = 0;
            if (!write) {
                FA_CHECK(fa_server_opt_get_state(ctx_, kv.first, nullptr, nullptr, nullptr, &steps));
            } else {
                ServerStatePart& sp = loaded_[kv.first];
                sp.n = kv.second.numel;
                for (auto* a : {&sp.x, &sp.m, &sp.v}) a->assign((size_t)sp.n, 0.0f);
                FA_CHECK(fa_server_opt_get_state(ctx_, kv.first, sp.x.data(), sp.m.data(), sp.v.data(), &steps));
                sp.steps = steps;
            }
            most = std::max<unsigned long long>(most, steps);
        }
        if (write && !write_server_state(o_.server_state, o_.server.rule, loaded_)) {
            std::cerr << "[aggregator] --server-state: cannot write " << o_.server_state << "\n";
            std::exit(1);
        }
        return most;
    }

    // --clip-norm: the round line's tail -- the receipts scaled down and left out this round and every
    // bucket's squared distances in slot order (17 significant digits: they read back to the same doubles) --
    // and, with --clip-state, every defined bucket's reference written to FILE.tmp and renamed over FILE (parts
    // read at startup and never defined in this run are carried over as read).
    std::string clip_tail() {
        std::ostringstream os;
        os << ",\"clip_norm\":" << o_.clip_norm << ",\"clipped\":" << clip_clipped_ << ",\"excluded\":" << clip_excluded_
           << ",\"clip_sumsq\":{";
        bool first = true;
        for (auto& kv : clip_q_) {
            os << (first ? "" : ",") << "\"" << kv.first << "\":[";
            first = false;
            for (size_t k = 0; k < kv.second.size(); ++k) {
                char buf[40];
                if (std::isfinite(kv.second[k])) snprintf(buf, sizeof buf, "%.17g", kv.second[k]);
                else snprintf(buf, sizeof buf, "\"%s\"", std::isnan(kv.second[k]) ? "nan" : "inf");
                os << (k ? "," : "") << buf;
            }
            os << "]";
        }
        os << "}";
        clip_clipped_ = clip_excluded_ = 0;
        clip_q_.clear();
        if (!o_.clip_state.empty()) {
            for (auto& kv : buckets_) {
                if (!kv.second.defined) continue;
                std::vector<float>& g = clip_loaded_[kv.first];
                g.assign(kv.second.numel, 0.0f);
                FA_CHECK(fa_clip_get_reference(ctx_, kv.first, g.data()));
            }
            if (!write_clip_state(o_.clip_state, clip_loaded_)) {
                std::cerr << "[aggregator] --clip-state: cannot write " << o_.clip_state << "\n";
                std::exit(1);
            }
        }
        return os.str();
    }

    // --dp-noise-multiplier: the round line's tail -- the multiplier, the stddev it gave (9 significant digits: it
    // reads back to the same float) and the generator round this round's buckets drew from (the most, if they
    // differ).
    std::string dp_tail() {
        unsigned long long used = 0;
        for (auto& kv : buckets_) {
            if (!kv.second.defined) continue;
            uint64_t next = 0;
            FA_CHECK(fa_noise_get_round(ctx_, kv.first, &next));
            if (next > 0) used = std::max<unsigned long long>(used, next - 1);
        }
        char buf[160];
        snprintf(buf, sizeof buf, ",\"dp_noise_multiplier\":%.17g,\"dp_stddev\":%.9g,\"dp_round\":%llu", o_.dp_z,
                 (double)dp_stddev_, used);
        return buf;
    }

    // --mode bulyan: the round line's tail -- per bucket the ids of the owners left out, the owners' ids in slot
    // order once.
    std::string bulyan_tail() {
        std::ostringstream os;
        os << ",\"bulyan_owners\":[";
        for (size_t k = 0; k < expected_.size(); ++k) os << (k ? "," : "") << expected_[k];
        os << "],\"bulyan_left_out\":{";
        bool first = true;
        for (auto& kv : bulyan_) {
            os << (first ? "" : ",") << "\"" << kv.first << "\":[";
            first = false;
            bool lead = true;
            for (size_t k = 0; k < kv.second.size(); ++k) {
                if (kv.second[k]) continue;
                os << (lead ? "" : ",") << expected_[k];
                lead = false;
            }
            os << "]";
        }
        os << "}";
        bulyan_.clear();
        return os.str();
    }

    // --geomed-iters: the round line's tail -- T and NU, the owners' ids in slot order once, and per bucket the valid
    // passes, the ids of the owners excluded, the last pass's squared distances (17 significant digits: they read back
    // to the same doubles; 0 for an excluded owner) and the final chain's weights (9 digits: the same floats).
    std::string geomed_tail() {
        std::ostringstream os;
        char buf[64];
        snprintf(buf, sizeof buf, "%.9g", (double)o_.geomed_nu);
        os << ",\"geomed_iters\":" << o_.geomed_iters << ",\"geomed_nu\":" << buf << ",\"geomed_owners\":[";
        for (size_t k = 0; k < expected_.size(); ++k) os << (k ? "," : "") << expected_[k];
        os << "]";
        for (int what = 0; what < 4; ++what) {
            os << (what == 0 ? ",\"geomed_passes\":{" : what == 1 ? ",\"geomed_excluded\":{" : what == 2 ? ",\"geomed_sumsq\":{"
                                                                                                      : ",\"geomed_weights\":{");
            bool first = true;
            for (auto& kv : geomed_) {
                os << (first ? "" : ",") << "\"" << kv.first << "\":";
                first = false;
                if (what == 0) {
                    os << kv.second.passes;
                    continue;
                }
                os << "[";
                bool lead = true;
                for (size_t k = 0; k < kv.second.included.size(); ++k) {
                    if (what == 1) {
                        if (kv.second.included[k]) continue;
                        os << (lead ? "" : ",") << expected_[k];
                    } else if (what == 2) {
                        const double v = kv.second.sumsq[k];
                        if (std::isfinite(v)) snprintf(buf, sizeof buf, "%.17g", v);
                        else snprintf(buf, sizeof buf, "\"%s\"", std::isnan(v) ? "nan" : "inf");
                        os << (lead ? "" : ",") << buf;
                    } else {
                        const double v = (double)kv.second.weights[k];
                        if (std::isfinite(v)) snprintf(buf, sizeof buf, "%.9g", v);
                        else snprintf(buf, sizeof buf, "\"%s\"", std::isnan(v) ? "nan" : "inf");
                        os << (lead ? "" : ",") << buf;
                    }
                    lead = false;
                }
                os << "]";
            }
            os << "}";
        }
        geomed_.clear();
        return os.str();
    }

    // --krum-f: the round line's tail -- per bucket the ids of the owners left out and every owner's score in
    // slot order (17 significant digits: they read back to the same doubles), the owners' ids in that order once.
    std::string krum_tail() {
        std::ostringstream os;
        os << ",\"krum_f\":" << o_.krum_f << ",\"krum_m\":" << o_.krum_m << ",\"krum_owners\":[";
        for (size_t k = 0; k < expected_.size(); ++k) os << (k ? "," : "") << expected_[k];
        os << "]";
        for (int pass = 0; pass < 2; ++pass) {
            os << (pass == 0 ? ",\"krum_left_out\":{" : ",\"krum_scores\":{");
            bool first = true;
            for (auto& kv : krum_) {
                os << (first ? "" : ",") << "\"" << kv.first << "\":[";
                first = false;
                bool lead = true;
                for (size_t k = 0; k < kv.second.scores.size(); ++k) {
                    if (pass == 0) {
                        if (kv.second.selected[k]) continue;
                        os << (lead ? "" : ",") << expected_[k];
                    } else {
                        char buf[40];
                        const double v = kv.second.scores[k];
                        if (std::isfinite(v)) snprintf(buf, sizeof buf, "%.17g", v);
                        else snprintf(buf, sizeof buf, "\"%s\"", std::isnan(v) ? "nan" : "inf");
                        os << (lead ? "" : ",") << buf;
                    }
                    lead = false;
                }
                os << "]";
            }
            os << "}";
        }
        krum_.clear();
        return os.str();
    }

    size_t bytes_in(int mp) { return buckets_[mp].bytes_in; }
    unsigned long long stale_dropped() const { return stale_dropped_; }
    unsigned long long ignored() const { return ignored_; }
    unsigned long long replaced() const { return replaced_; }
    unsigned long long clock_back() const { return clock_back_; }

    // The data owners whose receipt of bucket mp has not arrived this round ("mp 2: 4 7 9").
    std::string missing(const std::vector<int>& mps) {
        std::ostringstream os;
        for (int mp : mps) {
            const auto& got = buckets_[mp].arrived;
            std::ostringstream ids;
            int n = 0;
            for (int c : expected_)
                if (!got.count(c)) ids << (n++ ? " " : "") << c;
            if (n) os << (os.tellp() > 0 ? "; " : "") << "part " << mp << ": " << n << " owner(s) [" << ids.str() << "]";
        }
        return os.str();
    }

    // The reductions of a phase's buckets as one batched launch (fa_reduce_parts: the last-part layers of
    // phase 2, aggregator.cpp:108-150, are one segment table); the following reduce() calls then only
    // copy each result into its reply.  With --eager the chains already ran as the receipts arrived.
    void reduce_all(const std::vector<int>& mps) {
        if (o_.eager || mps.size() < 2) return;
        // parts whose receipts the library keeps to read in place (small pinned receipts, fa_bucket_host_read):
        // each finalize then reduces straight into its reply, one round trip per part instead of a launch here
        // and a copy there.  Asked of the library, which alone knows every condition (the environment, the
        // frames' alignment and pinning); when some part is not kept, the batched launch covers them all.
        if (std::all_of(mps.begin(), mps.end(), [&](int mp) {
                int kept = 0;
                FA_CHECK(fa_bucket_host_read(ctx_, mp, &kept));
                return kept == 1;
            }))
            return;
        const auto t0 = std::chrono::steady_clock::now();
        FA_CHECK(fa_reduce_parts(ctx_, (int)mps.size(), mps.data(), nullptr, nullptr));
        st_.finalize_s += secs_since(t0);
    }

    // Host-side time split since the last call: archive parse + slot staging (absorb), the GPU
    // reduction incl. its D2H copy (finalize), the reply archive + frame (frame).
    struct Stats {
        double absorb_s = 0, finalize_s = 0, frame_s = 0;
    };
    Stats take_stats() {
        Stats s = st_;
        st_ = Stats{};
        return s;
    }

private:
    struct Rec {  // one parameter record: where it lies in the archive, its bytes, where they go in the bucket
        size_t off = 0, bytes = 0, at = 0;
        bool operator==(const Rec& o) const { return off == o.off && bytes == o.bytes && at == o.at; }
    };
    using Recs = std::shared_ptr<const std::vector<Rec>>;
    struct Stream {
        std::shared_ptr<Inflight> in;
        int slot = -1;           // the slot it streams into (-1: none yet)
        bool cancelled = false;  // a receipt of its (owner, bucket) landed whole: never streamed again
        Recs recs;               // the layout it streams by (the bucket's at the time it was claimed)
        size_t next = 0;         // records sent so far
    };

    static Recs records_of(const Receipt& r, const std::vector<const void*>& ptrs, const std::vector<size_t>& bytes) {
        auto v = std::make_shared<std::vector<Rec>>();
        size_t at = 0;
        for (size_t i = 0; i < ptrs.size(); ++i) {
            v->push_back(Rec{(size_t)((const uint8_t*)ptrs[i] - r.blob()), bytes[i], at});
            at += bytes[i];
        }
        return v;
    }

    void intake() {
        for (auto& in : net_->take_new_streams()) streams_.push_back(Stream{in});
    }

    Stream take_stream(const Receipt& r) {
        intake();
        for (auto it = streams_.begin(); it != streams_.end(); ++it)
            if (it->in->buf.get() == r.frame.get()) {
                Stream s = *it;
                streams_.erase(it);
                return s;
            }
        return Stream{};
    }

    void cancel_streams(int owner, int mp) {
        for (auto& s : streams_)
            if (s.in->client_id == owner && s.in->model_part == mp) {
                s.slot = -1;
                s.cancelled = true;
            }
    }

    void claim(Stream& s) {
        const Inflight& in = *s.in;
        if (!phase_mps_.count(in.model_part) || !in.buf->pinned) return;
        auto bi = buckets_.find(in.model_part);
        if (bi == buckets_.end() || !bi->second.defined) return;
        Bucket& b = bi->second;
        if (!b.recs || b.recs->empty() || b.recs_len != in.blob_len || b.arrived.count(in.client_id)) return;
        auto si = slots_.find(in.client_id);
        if (si == slots_.end()) return;  // an owner not seen yet takes its slot when its receipt lands
        for (auto& o : streams_)
            if (&o != &s && o.slot >= 0 && o.in->client_id == in.client_id && o.in->model_part == in.model_part) return;
        s.slot = si->second;
        s.recs = b.recs;
        s.next = 0;
        b.held.push_back(in.buf);  // DMA'd from until the bucket is finalized, whatever becomes of the frame
    }

    void feed(Stream& s, size_t have) {
        const Inflight& in = *s.in;
        while (s.next < s.recs->size()) {
            const Rec& rc = (*s.recs)[s.next];
            if (in.blob_off + rc.off + rc.bytes > have) break;
            FA_CHECK(fa_submit_piece_pinned(ctx_, in.model_part, s.slot, rc.at, in.buf->data() + in.blob_off + rc.off,
                                            rc.bytes));
            streamed_bytes_ += rc.bytes;
            ++s.next;
        }
    }

    struct Bucket {
        bool defined = false;
        size_t numel = 0, bytes_in = 0;
        int elem = 4;  // bytes per parameter element: 4 fp32, 2 bf16 / fp16
        ParamDtype dtype = ParamDtype::F32;  // what the bucket was defined with; a receipt of another is refused
        Recs recs;            // the parameter records of the last pinned receipt (the streaming layout)
        size_t recs_len = 0;  // ... for archives of this length
        Receipt last;         // the last full receipt, across rounds: the reply's template
        bool reduced = false; // a round of this bucket was reduced: its output can take an MX8 update
        std::vector<std::shared_ptr<const Bytes>> held;  // pinned frames DMA'd from, until finalize
        std::set<int> arrived;  // client ids received this round
        std::map<int, Receipt> mx8_from;  // --mx8-reply: this round's MX8 receipts by owner, their replies' templates
    };

    int slot_of(int client) {
        auto it = slots_.find(client);
        if (it == slots_.end()) {  // an id outside the expected list takes the first slot nobody claimed
            int s = 0;
            while (s < o_.data_owners && claimed_[s]) ++s;
            if (s == o_.data_owners) {
                std::cerr << "[aggregator] more distinct clients than -d " << o_.data_owners << "\n";
                std::exit(1);
            }
            for (auto kv = slots_.begin(); kv != slots_.end();) kv = kv->second == s ? slots_.erase(kv) : std::next(kv);
            it = slots_.insert({client, s}).first;
        }
        claimed_[it->second] = 1;
        return it->second;
    }

    float weight_of(int client) const {
        if (o_.samples.empty()) return 1.0f / (float)o_.data_owners;
        double total = 0;
        for (auto& kv : o_.samples) total += kv.second;
        auto it = o_.samples.find(client);
        return it == o_.samples.end() ? 0.0f : (float)(it->second / total);
    }

    Options o_;
    NetLayer* net_;
    fa_ctx* ctx_ = nullptr;
    std::map<int, Bucket> buckets_;
    ServerState loaded_;  // --server-state: as read at startup, then as last written
    ClipState clip_loaded_;  // --clip-state: likewise
    // --clip-norm: this round's clipped and excluded receipts and each bucket's squared distances (clip_tail)
    unsigned long long clip_clipped_ = 0, clip_excluded_ = 0;
    std::map<int, std::vector<double>> clip_q_;
    float dp_stddev_ = 0.0f;  // --dp-noise-multiplier: the stddev given to the context
    // --krum-f: this round's scores and selection flags of each bucket, in slot order (krum_tail)
    struct KrumRound {
        std::vector<double> scores;
        std::vector<int> selected;
    };
    std::map<int, KrumRound> krum_;
    // --geomed-iters: this round's valid passes, final flags, last-pass distances and final weights of each bucket, in
    // slot order (geomed_tail)
    struct GeomedRound {
        int passes = 0;
        std::vector<int> included;
        std::vector<double> sumsq;
        std::vector<float> weights;
    };
    std::map<int, GeomedRound> geomed_;
    std::map<int, std::vector<int>> bulyan_;  // --mode bulyan: this round's pick flags of each bucket, in slot order
    std::map<int, int> slots_;  // client id -> slot
    std::vector<char> claimed_;  // slot -> an arrived client holds it
    std::vector<int> expected_;  // the data owners' ids in slot order
    Stats st_;
    ReceiptLedger ledger_;
    // cumulative receipt accounting, printed with every round
    unsigned long long stale_dropped_ = 0, ignored_ = 0, replaced_ = 0, clock_back_ = 0;
    std::vector<Stream> streams_;
    std::set<int> phase_mps_;
    unsigned long long streamed_ = 0, stream_fallbacks_ = 0, streamed_bytes_ = 0;
    unsigned long long mx8_receipts_ = 0, mx8_bytes_ = 0;  // --mx8: this round's
    unsigned long long mx8_replies_ = 0, mx8_bytes_out_ = 0, mx8_nan_blocks_ = 0;  // --mx8-reply: this round's
};

// The next receipt, with the failure detection the reference lacks (its receive loop blocks forever on a
// data owner that died, network_layer.cpp:654-665): every stall_report_s of silence names the owners still
// missing in this phase; after receipt_timeout_s of silence (if set) the aggregator exits with code 3.  Bytes
// of a streamed frame arriving count as activity.  While it waits, the frames still arriving are streamed to
// their slots (Aggregator::pump).
Receipt wait_receipt(NetLayer& net, const Options& o, Aggregator& agg, const std::vector<int>& mps, int round,
                     int phase) {
    static uint64_t gen = 0;  // the network layer's progress counter, as last seen (one consumer)
    Receipt r;
    auto last = std::chrono::steady_clock::now();
    int reports = 0;
    for (;;) {
        agg.pump();
        const double silent = secs_since(last);
        double wait = (reports + 1) * o.stall_report_s - silent;
        if (o.receipt_timeout_s > 0) wait = std::min(wait, o.receipt_timeout_s - silent);
        const int ev = net.wait_event(&r, &gen, std::max(1, (int)(wait * 1000)));
        if (ev == 1) return r;
        if (ev == 2) {  // progress: a frame is arriving
            last = std::chrono::steady_clock::now();
            reports = 0;
            continue;
        }
        const double now_silent = secs_since(last);
        const bool give_up = o.receipt_timeout_s > 0 && now_silent >= o.receipt_timeout_s - 1e-3;
        if (!give_up && now_silent < (reports + 1) * o.stall_report_s - 1e-3) continue;
        ++reports;
        std::cerr << "[aggregator] round " << round << " phase " << phase << ": no receipt for " << now_silent
                  << " s; missing " << agg.missing(mps) << (give_up ? "; giving up (--receipt-timeout)" : "")
                  << "\n";
        if (give_up) {
            net.stop();
            std::exit(3);
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    if (!parse_args(argc, argv, &o)) {
        usage();
        return 2;
    }
    // --server-state is read before any socket or device is opened: a file of another format or rule is a
    // mistake in the command line
    ServerState server_state;
    if (!o.server_state.empty()) {
        std::string why;
        if (!read_server_state(o.server_state, o.server.rule, &server_state, &why)) {
            std::cerr << "--server-state " << o.server_state << ": " << why << "\n";
            usage();
            return 2;
        }
    }
    ClipState clip_state;  // likewise
    if (!o.clip_state.empty()) {
        std::string why;
        if (!read_clip_state(o.clip_state, &clip_state, &why)) {
            std::cerr << "--clip-state " << o.clip_state << ": " << why << "\n";
            usage();
            return 2;
        }
    }
    if (o.mode == FA_TRIMMED && !o.samples.empty())
        std::cerr << "[aggregator] warning: --samples is ignored with --mode trimmed|median (the rule has no weights)\n";
    // pinned frame buffers: receipts DMA'd from, replies DMA'd into -- small ones too (from 4 KiB): a small
    // model's receipt then goes to its slot by one DMA instead of a copy into the staging chunks first, and
    // its reply comes back the same way (BASELINE C1)
    std::shared_ptr<BufferPool> pool;
    if (o.pinned) {
        pool = BufferPool::create(
            [](size_t n) -> char* {
                void* p = nullptr;
                return fa_host_alloc(n, &p) == FA_OK ? (char*)p : nullptr;
            },
            [](char* p) { fa_host_free(p); }, true, 4096);
        set_frame_allocator([pool](size_t n) { return pool->get(n); });
    }
    NetLayer net(o.id, RoutingTable(o.port_base), o.senders);
    net.set_link_mbps(o.link_mbps);
    net.set_rx_concurrency(o.rx_concurrency);
    if (o.pinned) net.set_streaming(o.stream_min);  // the records are DMA'd from the pinned frame as it fills
    std::string err;
    if (o.discover && !net.find_init(600, &err)) {
        std::cerr << "[aggregator] discovery failed: " << err << "\n";
        return 1;
    }
    if (!net.start()) {
        std::cerr << "[aggregator] cannot listen on port " << net.routes().port_for(o.id) << "\n";
        return 1;
    }
    std::cerr << "[aggregator] node " << o.id << " listening on " << net.listen_port() << "\n";

    Message refactor = net.next_refactor();  // aggregator.cpp:52-53
    const int L = o.last_layers > 0 ? o.last_layers : last_part_layers(refactor.model_name, refactor.start);
    std::cerr << "[aggregator] refactor: model " << refactor.model_name << "/" << refactor.model_type << " start "
              << refactor.start << " end " << refactor.end << " -> " << L << " last-part layer(s)\n";
    Aggregator agg(o, &net, refactor.data_owners, std::move(server_state), std::move(clip_state));

    // the round line names the rule only where it is not a mean (lines of the other modes stay as they were)
    const std::string mode_tail =
        o.bulyan             ? ",\"mode\":\"bulyan\",\"bulyan_f\":" + std::to_string(o.bulyan_f)
        : o.mode == FA_TRIMMED ? ",\"mode\":\"trimmed\",\"trim\":" + std::to_string(o.trim)
                             : std::string();
    for (int round = 0; o.rounds < 0 || round < o.rounds; ++round) {
        // phase 1: model part 1 from every data owner (aggregator.cpp:59-93)
        // Receipt accounting (the reference counts raw receipts, aggregator.cpp:59-92 / :112-149): a phase
        // ends when every data owner's receipt of every bucket of the phase is in, counted as distinct
        // (owner, bucket) pairs, so a retransmitted receipt replaces its slot instead of ending the phase
        // early with another owner missing.  A receipt of the other phase is always a retransmission of an
        // earlier one: a data owner sends its last-part layers only after it has received the phase-1 reply
        // (data_owner.cpp:228-245), which goes out after phase 1 ends, and its next part 1 only after every
        // phase-2 reply, which goes out after phase 2 ends.  So it is ignored (named in the log), never carried
        // into a later phase, where it would stand for a receipt its owner has not sent yet.  A late copy of
        // the SAME phase's bucket from an earlier round is a byte copy of a receipt already reduced, caught by
        // its (t_start, length, content) key and dropped (ReceiptLedger, host/receipts.h).  The round line
        // counts, cumulatively: stale_dropped (byte copies, either phase), ignored (other-phase receipts that
        // are not copies), replaced (retransmissions within a phase), clock_back (owner clocks that went back).
        auto t0 = std::chrono::steady_clock::now();
        agg.set_phase({1});
        int received = 0;
        while (received < o.data_owners) {
            Receipt r = wait_receipt(net, o, agg, {1}, round, 1);
            if (r.model_part != 1) {
                agg.other_phase(r, 1);
                continue;
            }
            if (agg.absorb(r)) ++received;
        }
        const double recv1 = secs_since(t0);
        const size_t in1 = agg.bytes_in(1);
        agg.end_phase();
        auto t1 = std::chrono::steady_clock::now();
        auto reply1 = agg.reduce(1);
        const double red1 = secs_since(t1);
        const auto s1 = agg.take_stats();
        agg.fan_out(reply1);

        // phase 2: every last-part layer from every data owner (:108-150)
        auto t2 = std::chrono::steady_clock::now();
        int got = 0;
        const int want = o.data_owners * L;
        std::vector<int> mps;
        for (int mp = 2; mp <= L + 1; ++mp) mps.push_back(mp);
        agg.set_phase(mps);
        while (got < want) {
            Receipt r = wait_receipt(net, o, agg, mps, round, 2);
            if (r.model_part == 1) {  // a retransmission of this round's part 1 (above), or a late copy
                agg.other_phase(r, 2);
                continue;
            }
            if (r.model_part < 2 || r.model_part > L + 1) {
                std::cerr << "[aggregator] unexpected model_part " << r.model_part << " in phase 2\n";
                continue;
            }
            if (agg.absorb(r)) ++got;
        }
        const double recv2 = secs_since(t2);
        size_t in2 = 0;
        for (int mp = 2; mp <= L + 1; ++mp) in2 += agg.bytes_in(mp);
        agg.end_phase();
        auto t3 = std::chrono::steady_clock::now();
        std::vector<Aggregator::Replies> replies;
        agg.reduce_all(mps);
        for (int mp : mps) replies.push_back(agg.reduce(mp));
        const double red2 = secs_since(t3);
        const auto s2 = agg.take_stats();
        auto t4 = std::chrono::steady_clock::now();
        for (auto& f : replies) agg.fan_out(f);  // :153-166, in layer order
        net.flush();
        const double send2 = secs_since(t4);
        // the replies are with the senders: the state is read back and stored off the reply path
        std::string server_tail;
        if (o.server.rule != FA_OPT_NONE) {
            char buf[128];
            snprintf(buf, sizeof buf, ",\"server_opt\":\"%s\",\"server_lr\":%g,\"server_steps\":%llu",
                     server_rule_name(o.server.rule), (double)o.server.lr, agg.save_server_state());
            server_tail = buf;
        }
        std::string mx8_tail;
        if (o.mx8) {
            const auto mx = agg.take_mx8();
            char buf[96];
            snprintf(buf, sizeof buf, ",\"mx8_receipts\":%llu,\"mx8_bytes_in\":%llu", mx.first, mx.second);
            mx8_tail = buf;
            if (o.mx8_reply) {
                const auto mo = agg.take_mx8_out();
                char obuf[128];
                snprintf(obuf, sizeof obuf, ",\"mx8_replies\":%llu,\"mx8_bytes_out\":%llu,\"mx8_nan_blocks\":%llu",
                         mo.replies, mo.bytes, mo.nan_blocks);
                mx8_tail += obuf;
            }
        }
        const std::string clip_tail = mx8_tail +
            (o.clip_given ? agg.clip_tail() : o.krum_given ? agg.krum_tail() : o.geomed_given ? agg.geomed_tail() : o.bulyan ? agg.bulyan_tail() : std::string()) + (o.dp_given ? agg.dp_tail() : std::string());
        printf("{\"round\":%d,\"phase1\":{\"receive_s\":%.6f,\"reduce_s\":%.6f,\"bytes_in\":%zu,"
               "\"absorb_s\":%.6f,\"finalize_s\":%.6f,\"frame_s\":%.6f},"
               "\"phase2\":{\"receive_s\":%.6f,\"reduce_s\":%.6f,\"bytes_in\":%zu,\"layers\":%d,"
               "\"absorb_s\":%.6f,\"finalize_s\":%.6f,\"frame_s\":%.6f,\"send_s\":%.6f},"
               "\"send_failures\":%llu,\"stale_dropped\":%llu,\"ignored\":%llu,\"replaced\":%llu,"
               "\"clock_back\":%llu,\"streamed\":%llu,\"stream_fallbacks\":%llu,\"streamed_bytes\":%llu%s%s%s}\n",
               round, recv1, red1, in1, s1.absorb_s, s1.finalize_s, s1.frame_s, recv2, red2, in2, L, s2.absorb_s,
               s2.finalize_s, s2.frame_s, send2, (unsigned long long)net.send_failures(), agg.stale_dropped(), agg.ignored(),
               agg.replaced(), agg.clock_back(), agg.streamed(), agg.stream_fallbacks(), agg.streamed_bytes(),
               mode_tail.c_str(), server_tail.c_str(), clip_tail.c_str());
        fflush(stdout);
    }
    net.stop();
    return 0;
}
