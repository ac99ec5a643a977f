// simulate_host.hpp -- the host side of rsem-simulate-reads before the first read is drawn: the files (simulation.cpp:188-209), theta
// (:94-115) and the tables every startSimulation builds (the four models and their parts: cited at each function).  Shared by the
// program (simulate_reads.cpp) and by tests/simulate_emu.cpp, which runs the device's attempt on the host over the same tables.
#pragma once
#include "../../../include/rsem_hip.h"
#include "model_host.hpp"
#include "results.hpp"

namespace rsemh {

inline std::vector<double> running(const double* v, size_t n) {  // a table's running sum, as every startSimulation forms it
    std::vector<double> c(v, v + n);
    for (size_t i = 1; i < n; i++) c[i] += c[i - 1];
    return c;
}
inline void running_rows(std::vector<double>& out, const std::vector<double>& p, size_t row) {
    out = p;
    for (size_t r = 0; r + row <= out.size(); r += row)
        for (size_t k = 1; k < row; k++) out[r + k] += out[r + k - 1];
}

// QProfile::startSimulation (QProfile.h:151-193) and Profile::startSimulation (Profile.h:163-205): running sums per row, and the rows of
// a quality (a position) without any mass get the behaviour of the rows that have some
inline std::vector<double> repaired_profile(const std::vector<double>& p) {
    std::vector<double> pc;
    running_rows(pc, p, kNCodes);
    const int N = kNCodes;
    for (size_t i = 0; i < p.size() / 25; i++) {
        const double* pi = p.data() + i * 25;
        double* ci = pc.data() + i * 25;
        double cp_sum = 0.0, cp_d = 0.0, cp_n = 0.0;
        for (int j = 0; j < N - 1; j++) {
            cp_sum += ci[j * N + N - 1];
            cp_d += pi[j * N + j];
            cp_n += pi[j * N + N - 1];
        }
        if (cp_sum == 0.0) continue;
        const double p_d = cp_d / cp_sum, p_n = cp_n / cp_sum;
        double p_o = (1.0 - p_d - p_n) / (N - 2);
        for (int j = 0; j < N - 1; j++) {
            if (ci[j * N + N - 1] > 0.0) continue;
            for (int k = 0; k < N; k++) {
                ci[j * N + k] = k == j ? p_d : (k == N - 1 ? p_n : p_o);
                if (k > 0) ci[j * N + k] += ci[j * N + k - 1];
            }
        }
        if (ci[(N - 1) * N + N - 1] == 0.0) {
            p_o = (1.0 - p_n) / (N - 1);
            for (int k = 0; k < N; k++) {
                ci[(N - 1) * N + k] = k < N - 1 ? p_o : p_n;
                if (k > 0) ci[(N - 1) * N + k] += ci[(N - 1) * N + k - 1];
            }
        }
    }
    return pc;
}

// everything rsem_sim_create takes, and what owns it
struct SimInputs {
    RefInfo R;
    Transcripts T;
    Model model;
    std::vector<double> eel, theta, theta_cdf, qc_init, qc_trans, pc, npc;
    std::vector<uint64_t> seq_off;
    std::string seq;
    rsem_sim_model sm;
    SimInputs() = default;
    SimInputs(const SimInputs&) = delete;  // sm points into the vectors
    SimInputs& operator=(const SimInputs&) = delete;
};

// in the reference's order, with its messages: the sequences, the transcripts, the model file ("Cannot open ..."), theta, the tables
inline void load_sim_inputs(SimInputs& in, const std::string& refName, const std::string& modelF, const std::string& resultsF, const char* theta0_text, bool verbose) {
    const int offsite = is_allele_specific(refName) ? 6 : 5;  // simulation.cpp:190
    in.R = load_refs(refName + ".seq", true);
    const RefInfo& R = in.R;
    if (verbose) printf("Refs.loadRefs finished!\n");
    const int M = R.M;
    in.T = load_transcripts(refName + ".ti");
    {
        FILE* fi = fopen(modelF.c_str(), "r");
        if (!fi) { fprintf(stderr, "Cannot open %s! It may not exist.\n", modelF.c_str()); exit(-1); }
        fclose(fi);
    }
    if (M < 1) die("%s.seq holds no transcript", refName.c_str());
    const double theta0 = atof(theta0_text);  // simulation.cpp:206
    Model& model = in.model;
    model.read(modelF, 0);
    if (model.type < 0 || model.type > 3) die("%s: a model type from 0 to 3 is expected", modelF.c_str());
    const bool fastq = model.hasQ(), paired = model.paired();

    // theta (simulation.cpp:94-115)
    in.eel = calc_eel(M, R, model.gld);
    const std::vector<double>& eel = in.eel;
    std::vector<double>& theta = in.theta;
    theta.assign(M + 1, 0.0);
    theta[0] = theta0;
    {
        MappedFile f;
        if (!f.open(resultsF)) die("Cannot open %s! It may not exist.", resultsF.c_str());
        const char* p = f.data;
        const char* end = f.data + f.size;
        auto line = [&](const char*& b, const char*& e) {
            b = p;
            const char* nl = p < end ? (const char*)memchr(p, '\n', end - p) : nullptr;
            e = nl ? nl : end;
            p = nl ? nl + 1 : end;
        };
        const char *b, *e;
        line(b, e);  // the column names
        double denom = 0.0;
        for (int i = 1; i <= M; i++) {
            line(b, e);
            const char* q = b;
            for (int j = 0; j < offsite; j++) {  // (a line with fewer columns: find_first_of gives npos, npos + 1 = 0, the search starts again)
                const char* tab = (const char*)memchr(q, '\t', e - q);
                q = tab ? tab + 1 : b;
            }
            const char* q2 = (const char*)memchr(q, '\t', e - q);
            const std::string cell(q, (q2 ? q2 : e) - q);
            theta[i] = atof(cell.c_str()) * eel[i];
            denom += theta[i];
        }
        if (!(denom > kEpsilon)) die("%s: no transcript with a TPM above 0 has an effective length", resultsF.c_str());
        for (int i = 1; i <= M; i++) theta[i] = theta[i] / denom * (1.0 - theta[0]);
    }

    // the tables of startSimulation
    rsem_sim_model& sm = in.sm;
    sm = rsem_sim_model{};
    sm.type = model.type; sm.M = M; sm.has_mld = model.has_mld ? 1 : 0; sm.est_rspd = model.rspd.est ? 1 : 0; sm.B = model.rspd.B;
    sm.g_lb = model.gld.lb; sm.g_ub = model.gld.ub; sm.m_lb = model.mld.lb; sm.m_ub = model.mld.ub; sm.prob_f = model.probF;
    in.theta_cdf = running(theta.data(), theta.size());
    std::vector<uint64_t>& seq_off = in.seq_off;
    seq_off.assign(M + 2, 0);
    std::string& seq = in.seq;
    const std::vector<double>& theta_cdf = in.theta_cdf;
    for (int i = 1; i <= M; i++) {
        if ((int)R.seq[i].size() < R.totLen[i]) die("%s.seq: transcript %d has %zu letters, %d are announced", refName.c_str(), i, R.seq[i].size(), R.totLen[i]);
        seq_off[i] = seq.size();
        seq += R.seq[i];
    }
    seq_off[M + 1] = seq.size();
    if (seq.empty()) seq.push_back('N');
    std::vector<double>&qc_init = in.qc_init, &qc_trans = in.qc_trans, &pc = in.pc, &npc = in.npc;
    if (fastq) {
        qc_init = running(model.qd_init.data(), kQSize);               // QualDist.h:116-130
        running_rows(qc_trans, model.qd_tran, kQSize);
        pc = repaired_profile(model.qpro);
        running_rows(npc, model.nq_p, kNCodes);                         // NoiseQProfile.h:153-166
        for (int i = 0; i < kQSize; i++)
            if (fabs(npc[i * 5 + 4]) < 1e-8) { npc[i * 5] = 0.25; npc[i * 5 + 1] = 0.5; npc[i * 5 + 2] = 0.75; npc[i * 5 + 3] = 1.0; npc[i * 5 + 4] = 1.0; }
    } else {
        pc = repaired_profile(model.pro);
        npc = running(model.np_p, kNCodes);                             // NoiseProfile.h:137-144
        sm.pro_len = model.proLen;
        const int longest = model.has_mld ? model.mld.ub : model.gld.ub;
        if (longest > model.proLen) die("%s: reads of up to %d bases, a profile of %d positions (Profile.h:211 would read past it)", modelF.c_str(), longest, model.proLen);
    }
    if (paired && model.gld.lb < model.mld.lb)
        die("%s: inserts from %d bases on, mates from %d: an insert shorter than every mate length is undefined in the reference (PairedEndQModel.h:415-417)", modelF.c_str(),
            model.gld.lb + 1, model.mld.lb + 1);
    sm.theta_cdf = theta_cdf.data(); sm.full_len = R.fullLen.data(); sm.tot_len = R.totLen.data(); sm.seq_off = seq_off.data(); sm.seq = (const uint8_t*)seq.data();
    sm.g_cdf = model.gld.cdf.data(); sm.m_cdf = model.has_mld ? model.mld.cdf.data() : nullptr;
    sm.r_pdf = model.rspd.pdf.data(); sm.r_cdf = model.rspd.cdf.data();
    sm.qc_init = fastq ? qc_init.data() : nullptr; sm.qc_trans = fastq ? qc_trans.data() : nullptr; sm.pc = pc.data(); sm.npc = npc.data();
}

}  // namespace rsemh
