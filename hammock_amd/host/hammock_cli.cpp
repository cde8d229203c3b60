// hammock_cli.cpp -- `hammock-hip greedy ...`: the C++ counterpart of
// `java -jar Hammock.jar greedy ...` (Hammock.java:142-172, :217-234, :392-437) that drives
// the same C ABI the Java shim binds.  Flags, defaults, log lines and result files follow the
// reference's greedy mode; everything after initial clustering (Clustal Omega MSAs, HMM stage)
// is out of scope.
//
// Extra flags that the reference does not have: --device <k> (HIP ordinal, default 0) and --devices a,b,.. (several
// GPUs of the node behind one context, the first is the root: hmk_create_multi).
// Extra modes that the reference does not have: search, assign, match, continue, merge, ... and scan (runSearch, runAssign, ...), each described
// above its run function.  Every run function is a list of the shared steps below (parseModeArgs ... writeRankedTable) and what is its own.
#include <deque>
#include <future>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <climits>

#include <malloc.h>

#include "hammock_host.hpp"
#include "hammock_targets.hpp"

using namespace hammock;

namespace {

const char *VERSION = "1.2.0";  // the Hammock version whose greedy mode this mirrors (Hammock.java:39)

std::string parentDir() {  // PARENT_DIR (Hammock.java:36): two levels above the binary
    char buf[PATH_MAX];
    const ssize_t n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
    std::string p = n > 0 ? std::string(buf, (size_t)n) : std::string("./hammock-hip");
    for (int k = 0; k < 2; k++) {
        const size_t s = p.find_last_of('/');
        p = s == std::string::npos ? std::string(".") : p.substr(0, s);
    }
    return p;
}

bool exists(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0; }

struct Options {
    // common (Hammock.java:40-67)
    std::string inputFileName, workingDirectory, matrixFile, labelString, tempDirectory = "/tmp";
    bool haveInput = false, haveDir = false, haveLabels = false;
    int nThreads = 4;
    int seed = 42;
    // greedy (Hammock.java:79-85)
    std::string inputType = "fasta", order = "size";
    bool haveThreshold = false, haveMaxShift = false, haveLimit = false;
    int sequenceClusteringThreshold = 0, shiftPenalty = 0, maxShift = 0, initialClustersLimit = 0;
    int cacheSizeLimit = 1;   // clinkage: -L is parsed and logged, never used (Hammock.java:89,1004-1008,459)
    int device = 0;
    std::vector<int> devices;   // --devices 0,1,..: pair space sharded over several GPUs
    int javaHashSet = 8;        // --java_hashset 8|7|6 (clinkage, merge): whose java.util.HashSet iteration order is emulated
    // the newer modes' own (parseModeArgs)
    std::string clustersFile, database, parentDir;
    bool haveClusters = false, haveDatabase = false, havePenalty = false, skipSingletons = false;
    int best = 0;
    bool haveScanTo = false;   // components: --scan_to T2, the last threshold of the scan (default: -g alone)
    int scanTo = 0;
    // search, greedy: --scorer shifted|global (parseScorerArgs); global: GlobalAlignmentScorer with --gap_open / --gap_extend
    bool haveScorer = false, globalScorer = false;
    int gapOpen = -5, gapExtend = -1;
    bool alignments = false;   // search --scorer global --alignments: the hits' gapped rows (hmk_align_pairs_global)
};

void parseCommonArgs(const std::vector<std::string> &args, Options &o) {  // Hammock.java:824-908
    o.parentDir = parentDir();
    o.matrixFile = o.parentDir + "/matrices/blosum62.txt";  // Hammock.java:45
    for (size_t i = 1; i < args.size(); i++) {
        const std::string &a = args[i];
        const bool more = args.size() > i + 1;
        if ((a == "-i" || a == "--input") && more) { o.inputFileName = args[++i]; o.haveInput = true; continue; }
        if ((a == "-d" || a == "--outputDirectory") && more) { o.workingDirectory = args[++i]; o.haveDir = true; continue; }  // :834
        if ((a == "-m" || a == "--matrix") && more) { o.matrixFile = args[++i]; continue; }
        if ((a == "-t" || a == "--threads") && more) {
            try { size_t u = 0; o.nThreads = std::stoi(args[i + 1], &u); if (u != args[i + 1].size()) throw 0; }
            catch (...) { throw HammockException("NumberFormatException: For input string: \"" + args[i + 1] + "\""); }
            i++;
            continue;
        }
        if ((a == "-l" || a == "--labels") && more) { o.labelString = args[++i]; o.haveLabels = true; continue; }
        if (a == "--temp" && more) { o.tempDirectory = args[i + 1]; }  // :903-905 (no skip, as in the reference)
        if (a == "--device" && more) { o.device = javaIntegerDecode(args[++i]); continue; }
        if (a == "--java_hashset" && more) {
            o.javaHashSet = javaIntegerDecode(args[++i]);
            if (o.javaHashSet != 8 && o.javaHashSet != 7 && o.javaHashSet != 6)
                throw CLIException("Error. --java_hashset may be 8 (Java 8 and later, the default), 7 (JDK 7u6 and later 7 updates) or 6 (JDK 6, JDK 7 before 7u6).");
            continue;
        }
        if (a == "--devices" && more) {
            o.devices.clear();
            std::string list = args[++i], tok;
            for (size_t b = 0; b <= list.size(); b++) {
                if (b == list.size() || list[b] == ',') { if (!tok.empty()) o.devices.push_back(javaIntegerDecode(tok)); tok.clear(); }
                else tok.push_back(list[b]);
            }
            if (o.devices.empty()) throw HammockException("--devices needs a comma separated list of HIP ordinals");
            continue;
        }
    }
}

void parseGreedyArgs(const std::vector<std::string> &args, Options &o) {  // Hammock.java:915-970
    for (size_t i = 1; i < args.size(); i++) {
        const std::string &a = args[i];
        const bool more = args.size() > i + 1;
        if ((a == "-f" || a == "--file_format") && more) { o.inputType = args[++i]; continue; }
        if ((a == "-g" || a == "--greedy_threshold" || a == "--alignment_threshold") && more) {
            o.sequenceClusteringThreshold = javaIntegerDecode(args[++i]); o.haveThreshold = true; continue;
        }
        if ((a == "-x" || a == "--max_shift") && more) { o.maxShift = javaIntegerDecode(args[++i]); o.haveMaxShift = true; continue; }
        if ((a == "-R" || a == "--order") && more) { o.order = args[++i]; continue; }
        if ((a == "-S" || a == "--seed") && more) { o.seed = javaIntegerDecode(args[++i]); continue; }
        if ((a == "-p" || a == "--gap_penalty") && more) { o.shiftPenalty = javaIntegerDecode(args[++i]); }
        else if (a == "--initial_clusters_limit" && more) { o.initialClustersLimit = javaIntegerDecode(args[++i]); o.haveLimit = true; }
    }
}

void parseClinkageArgs(const std::vector<std::string> &args, Options &o) {  // Hammock.java:972-1011
    for (size_t i = 1; i < args.size(); i++) {
        const std::string &a = args[i];
        const bool more = args.size() > i + 1;
        if ((a == "-f" || a == "--file_format") && more) { o.inputType = args[++i]; continue; }
        if ((a == "-x" || a == "--max_shift") && more) { o.maxShift = javaIntegerDecode(args[++i]); o.haveMaxShift = true; continue; }
        if ((a == "-p" || a == "--gap_penalty") && more) { o.shiftPenalty = javaIntegerDecode(args[++i]); }
        if ((args[i] == "-g" || args[i] == "--greedy_threshold" || args[i] == "--alignment_threshold") && args.size() > i + 1) {
            o.sequenceClusteringThreshold = javaIntegerDecode(args[++i]); o.haveThreshold = true;
        }
        if ((args[i] == "-L" || args[i] == "--cache_size_limit") && args.size() > i + 1) { o.cacheSizeLimit = javaIntegerDecode(args[++i]); }
    }
}

// search, greedy: --scorer shifted|global, --gap_open, --gap_extend.  With the global scorer the shift parameters have no meaning
// (-x, -p are errors), the penalties must satisfy the library's condition, and the pass runs on one device.
void parseScorerArgs(const std::vector<std::string> &args, Options &o) {
    bool shiftArgs = false;
    for (size_t i = 1; i < args.size(); i++) {
        const std::string &a = args[i];
        const bool more = args.size() > i + 1;
        if (a == "--scorer" && more) {
            const std::string &name = args[++i];
            if (name != "shifted" && name != "global") throw CLIException("Error. --scorer may be either \"shifted\" or \"global\".");
            o.haveScorer = true;
            o.globalScorer = name == "global";
        } else if (a == "--gap_open" && more) o.gapOpen = javaIntegerDecode(args[++i]);
        else if (a == "--gap_extend" && more) o.gapExtend = javaIntegerDecode(args[++i]);
        else if (a == "--alignments") o.alignments = true;
        else if (a == "-x" || a == "--max_shift" || a == "-p" || a == "--gap_penalty") shiftArgs = true;
    }
    if (o.alignments && !o.globalScorer) throw CLIException("Error. --alignments needs --scorer global (the gapped rows are that scorer's alignments).");
    if (!o.globalScorer) return;
    if (shiftArgs) throw CLIException("Error. -x (--max_shift) and -p (--gap_penalty) have no meaning with --scorer global (--gap_open, --gap_extend).");
    if (o.gapOpen < -127 || o.gapOpen > o.gapExtend || o.gapExtend > 0)
        throw CLIException("Error. --scorer global needs -127 <= --gap_open <= --gap_extend <= 0.");
    if (!o.devices.empty()) throw CLIException("Error. --devices is not available with --scorer global (the pass runs on one device, --device).");
}

void logScorer(const Options &o, const Logger &logger) {   // (only when --scorer was given: every other run logs as before)
    if (!o.haveScorer) return;
    logger.logAndStderr(o.globalScorer ? "Scorer: global (global alignment, affine gap). Gap open penalty: " + std::to_string(o.gapOpen) +
                                             ", gap extend penalty: " + std::to_string(o.gapExtend)
                                       : std::string("Scorer: shifted"));
}

void printHelp() {  // Hammock.java:295-320 (greedy-relevant part)
    std::cerr << "\nhammock-hip: MI355X-native greedy and clinkage modes of Hammock version " << VERSION << "\n\n"
              << "Synopsis: hammock-hip <greedy|clinkage> <param1> <param2> ...\n"
              << "          hammock-hip greedy ... [--scorer shifted|global] [--gap_open <int>] [--gap_extend <int>]\n"
              << "          hammock-hip search -i <queries> --database <references> -d <directory> [-f fasta|tab] [-m <file>] [-x <int>]\n"
              << "                      [-p <int>] [-g <int>] [--best <int>] [--scorer shifted|global] [--gap_open <int>] [--gap_extend <int>]\n"
              << "                      [--alignments] [--device <int>]\n"
              << "          hammock-hip assign -i <new sequences> --clusters <initial_clusters_sequences.tsv> -d <directory> [--best <int>]\n"
              << "                      [--skip_singletons] [-f fasta|tab] [-m <file>] [-x <int>] [-p <int>] [-g <int>] [--device <int>]\n"
              << "          hammock-hip continue -i <new sequences> --clusters <initial_clusters_sequences.tsv> -d <directory> [-f fasta|tab]\n"
              << "                      [-m <file>] [-x <int>] [-p <int>] [-g <int>] [-R <order>] [-S <int>] [-l <labels>] [--device <int>]\n"
              << "          hammock-hip match -i <query clusters.tsv> --clusters <initial_clusters_sequences.tsv> -d <directory> [--best <int>]\n"
              << "                      [--skip_singletons] [-m <file>] [-x <int>] [-p <int>] [-g <int>] [--device <int>]\n"
              << "          hammock-hip merge -i <clusters.tsv> [--clusters <other clusters.tsv>] -d <directory> [--skip_singletons] [-m <file>]\n"
              << "                      [-x <int>] [-p <int>] [-g <int>] [--java_hashset <int>] [--device <int>]\n"
              << "          hammock-hip check -i <clusters.tsv> -d <directory> [--skip_singletons] [-m <file>] [-x <int>] [-p <int>] [-g <int>]\n"
              << "                      [--device <int>]\n"
              << "          hammock-hip split -i <clusters.tsv> -d <directory> [-m <file>] [-x <int>] [-p <int>] [-g <int>] [--java_hashset <int>]\n"
              << "                      [--device <int>]\n"
              << "          hammock-hip align -i <clusters.tsv> -d <directory> [--skip_singletons] [-m <file>] [-x <int>] [-p <int>] [--device <int>]\n"
              << "          hammock-hip align -i <clusters.tsv> -d <directory> --scorer global [--gap_open <int>] [--gap_extend <int>] [--skip_singletons]\n"
              << "                      [-m <file>] [--device <int>]\n"
              << "          hammock-hip profile -i <clusters.tsv> -d <directory> --frequency_matrix <file> [--background <file>] [--min_ic <float>]\n"
              << "                      [--max_gap_proportion <float>] [--min_conserved_positions <int>] [--max_inner_gaps <int>] [--skip_singletons]\n"
              << "                      [-m <file>] [-x <int>] [-p <int>] [--device <int>]\n"
              << "          hammock-hip components -i <sequences> -d <directory> [-g <int>] [--scan_to <int>] [-f fasta|tab] [-m <file>] [-x <int>]\n"
              << "                      [-p <int>] [-l <labels>] [--device <int>]\n"
              << "          hammock-hip density -i <sequences> -d <directory> [-g <int>] [--min_neighbors <int>] [--scan_to <int>] [--pick <int>]\n"
              << "                      [-f fasta|tab] [-m <file>] [-x <int>] [-p <int>] [-l <labels>] [--device <int>]\n"
              << "          hammock-hip sweep -i <sequences> -d <directory> [-g <int>] [--scan_to <int>] [--pick <int>] [-f fasta|tab] [-m <file>]\n"
              << "                      [-x <int>] [-p <int>] [-R <order>] [-S <int>] [-l <labels>] [--initial_clusters_limit <int>] [--device <int>]\n"
              << "          hammock-hip orders -i <sequences> -d <directory> [-R <order>] [--random_orders <int>] [-S <int>] [--min_support <int>] [--pairs]\n"
              << "                      [-g <int>] [-f fasta|tab] [-m <file>] [-x <int>] [-p <int>] [-l <labels>] [--initial_clusters_limit <int>] [--device <int>]\n"
              << "          hammock-hip representatives -i <sequences> -d <directory> [-g <int>] [--scan_to <int>] [-f fasta|tab] [-m <file>]\n"
              << "                      [-x <int>] [-p <int>] [-R <order>] [-S <int>] [-l <labels>] [--device <int>]\n"
              << "          hammock-hip survey -i <sequences> -d <directory> [-g <int>] [--database <sequences>] [-f fasta|tab] [-m <file>] [-x <int>]\n"
              << "                      [-p <int>] [-l <labels>] [--device <int>]\n"
              << "          hammock-hip scan -i <peptides> --targets <proteins.fa> -d <directory> [-g <int>] [-x <int>] [-p <int>] [--all_windows]\n"
              << "                      [-f fasta|tab] [-m <file>] [--device <int>]\n"
              << "          hammock-hip separation -i <clusters.tsv> -d <directory> [--skip_singletons] [-m <file>] [-x <int>] [-p <int>] [-l <labels>]\n"
              << "                      [--device <int>]\n\n"
              << "-i, --input <file>\n\tA path to an input file\n\n"
              << "-d, --output_directory <directory>\n\tA directory to store all output files in\n\n"
              << "-t, --threads <int>\n\tAccepted for compatibility (the GPU path ignores it)\n\n"
              << "-l, --labels <str,str,str...>\n\tA list of sequence labels to use\n\n"
              << "-f, --file_format <[fasta,tab]>\n\tThe file format of input file specified by -i\n\n"
              << "-m, --matrix <file>\n\tA path to a substitution matrix file\n\n"
              << "-g, --alignment_threshold, (--greedy_threshold) <int>\n\tMinimal score needed for a sequence to join a cluster\n\n"
              << "-x, --max_shift <int>\n\tMaximal sequence-sequence shift. A nonnegative int\n\n"
              << "-p, --gap_penalty <int>\n\tThe penalty for each position of the sequence-sequence shift. A nonpositive int\n\n"
              << "-R, --order [size, alphabetic, random, input, <label>]\n\tThe order of sequences during greedy clustering\n\n"
              << "-S, --seed <int>\n\tA seed to make random processes deterministic (if -R random is in use)\n\n"
              << "--initial_clusters_limit <int>\n\tThe max. number of clusters resulting from gredy clustering\n\n"
              << "-L, --cache_size_limit <int>\n\t(clinkage) accepted and logged; has no effect, as in the reference\n\n"
              << "--scorer <[shifted,global]>\n\t(search, greedy) the pair score: shifted (default) = ShiftedScorer with -x and -p; global = the optimal global\n\talignment score of the two whole sequences under the matrix with an affine gap (end gaps charged); -x and -p are errors with it.\n\tsearch then writes the columns query, target, score;\n\t(align) global: gapped rows, a centre-star merge of the members' global alignments with their cluster's centre\n\n"
              << "--alignments\n\t(search --scorer global) two more columns behind score, query_row and target_row: the hit's gapped alignment\n\n"
              << "--gap_open <int>\n\t(--scorer global) the penalty added for the first position of a gap (default -5); -127 <= --gap_open <= --gap_extend <= 0\n\n"
              << "--gap_extend <int>\n\t(--scorer global) the penalty added for every further position of a gap (default -1)\n\n"
              << "--device <int>\n\tHIP device ordinal (default 0)\n\n"
              << "--devices <int,int,...>\n\tShard the pair space over several GPUs of the node (the first one runs the merge)\n\n"
              << "--database <file>\n\t(search) the reference sequences every query (-i) is scored against;\n\t(survey) score the input against these sequences instead of against itself\n\n"
              << "--targets <file>\n\t(scan) the long sequences (an antigen, a proteome) the peptides of -i are slid along: a FASTA file whose sequences may\n\tspan lines, named by the header up to the first white space, never merged; 33 to 1,048,576 residues each\n\n"
              << "--all_windows\n\t(scan) one line per window at or above -g instead of one per (peptide, target) with its best window\n\n"
              << "--best <int>\n\t(search) keep only the best 1..32 hits of each query; (assign, match) report the best 1..32 feasible clusters (default 1)\n\n"
              << "--clusters <file>\n\t(assign, continue, match) the existing clusters, a cluster file as greedy writes it (initial_clusters_sequences.tsv);\n\t(merge) a second cluster file: its clusters keep their ids, the -i file's are renumbered behind them\n\n"
              << "--scan_to <int>\n\t(components) the last threshold of the scan: component_levels.tsv gets one line per threshold from -g to this one\n\t(at most 255 above -g; default: -g alone);\n\t(sweep) the last threshold of the sweep: greedy_levels.tsv gets one line per threshold from -g to this one;\n\t(representatives) the last threshold: representative_levels.tsv gets one line per threshold from -g to this one;\n\t(density) the last threshold: density_levels.tsv gets one line per threshold from -g to this one\n\n"
              << "--pick <int>\n\t(sweep) the threshold of the sweep whose clustering is written as the stage-1 files (default: -g);\n\t(density) the threshold whose clusters are written as density_members.tsv and the stage-1 files (default: -g)\n\n"
              << "--random_orders <int>\n\t(orders) how many random orders are clustered beside the -R order, 0 to 255 (default 9): order k is -R random with the seed\n\t-S + k - 1\n\n"
              << "--min_support <int>\n\t(orders) the consensus clusters are the components of the pairs that share a cluster in at least this many valid orders\n\t(default 0: in every valid order)\n\n"
              << "--pairs\n\t(orders) also write pair_support.tsv: every pair that shares a cluster in at least one order, with its support\n\n"
              << "--min_neighbors <int>\n\t(density) a sequence with at least this many neighbours (itself not counted) is core (default 3)\n\n"
              << "--frequency_matrix <file>\n\t(profile) required: a row-normalised frequency matrix q_ij in the format of Hammock's settings/misc/blosum62.freq_rownorm\n\t('#' comment lines, one header line of letters, tab-separated rows); hammock-hip ships no such table\n\n"
              << "--background <file>\n\t(profile) one line of 20 background probabilities in the letter order of the frequency matrix file (default: 0.05 throughout,\n\tthe equiprobable model the information content uses).  Hammock's own table is the array at Statistics.java:25-28: pass it in a file\n\tto get Hammock's KLD numbers\n\n"
              << "-k, --min_ic <float>\n\t(profile) minimal information content of a conserved MSA position (default 1.2)\n\n"
              << "-y, --max_gap_proportion <float [0, 1]>\n\t(profile) maximal proportion of gaps in a conserved MSA position (default 0.2)\n\n"
              << "-h, --min_conserved_positions <int>\n\t(profile) a cluster passes with at least this many conserved positions (default: a third of the mean sequence length)\n\n"
              << "-u, --max_inner_gaps <int>\n\t(profile) above 0, non-match positions may lie between match states (default 0)\n\n"
              << "--skip_singletons\n\t(assign, match, merge) only clusters of more than one unique sequence are candidates;\n\t(check) clusters of one unique sequence are left out of cluster_linkage.tsv;\n\t(align, profile) clusters of one unique sequence are left out of cluster_centers.tsv (profile: and of cluster_profiles.tsv,\n\tposition_profiles.tsv and member_kld.tsv);\n\t(separation) clusters of one unique sequence are neither members nor candidates for the nearest cluster\n\n"
              << "--java_hashset <8|7|6>\n\t(clinkage, merge, split) whose java.util.HashSet iteration order picks the chain starts and orders the result: 8 = Java 8 and\n\tlater (default), 7 = JDK 7u6 and later updates of 7, 6 = JDK 6 and JDK 7 before 7u6\n\n";
}

std::string labelsToString(bool have, const std::vector<std::string> &labels) {  // List.toString() / "null"
    if (!have) return "null";
    std::string s = "[";
    for (size_t k = 0; k < labels.size(); k++) s += (k ? ", " : "") + labels[k];
    return s + "]";
}

// Hammock.java:1421-1427 (the list's shortest length comes from the one summary pass; the mean length, :1554-1563, too)
int checkMaxShift(const SequenceListSummary &summary, int maxShift) { return std::min(maxShift, summary.minLength - 1); }

// ---- the steps the modes' run functions are made of --------------------------------------------------------------------
using ContextFuture = std::shared_future<std::shared_ptr<NativeContext>>;

long long millisSince(std::chrono::steady_clock::time_point time0) {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - time0).count();
}

// The newer modes' arguments: greedy's (-f -g -x -R -S -p) and their own.  Each parser walks all of args on its own, as the
// reference's do; only --clusters, --database, --best and --scan_to take their value here.  bestDefault < 0: the mode has no --best.
void parseModeArgs(const std::vector<std::string> &args, Options &o, int bestDefault) {
    parseGreedyArgs(args, o);
    o.best = std::max(bestDefault, 0);
    for (size_t i = 1; i < args.size(); i++) {
        const bool more = args.size() > i + 1;
        if (args[i] == "--clusters" && more) { o.clustersFile = args[++i]; o.haveClusters = true; }
        else if (args[i] == "--database" && more) { o.database = args[++i]; o.haveDatabase = true; }
        else if (args[i] == "--best" && more && bestDefault >= 0) {
            o.best = javaIntegerDecode(args[++i]);
            if (o.best < 1 || o.best > 32) throw CLIException("Error. --best may be 1 to 32.");
        } else if (args[i] == "--scan_to" && more) { o.scanTo = javaIntegerDecode(args[++i]); o.haveScanTo = true; }
        else if (args[i] == "--skip_singletons") o.skipSingletons = true;
        else if ((args[i] == "-p" || args[i] == "--gap_penalty") && more) o.havePenalty = true;
    }
}

void requireInput(const Options &o) {  // checkCommonArgs, Hammock.java:1207-1211
    if (!o.haveInput) throw CLIException("Error. Parameter input file (-i or --input) missing with no default.");
}
void requireClusters(const Options &o) {
    if (!o.haveClusters) throw CLIException("Error. Parameter cluster file (--clusters) missing with no default.");
}
void requireOneDevice(const Options &o, const std::string &mode, const std::string &aRun) {
    if (!o.devices.empty())
        throw CLIException("Error. --devices is not available in mode " + mode + " (" + aRun + " runs on one device, --device).");
}
void requireFastaOrTab(const Options &o, const std::string &mode) {
    if (!(o.inputType == "fasta" || o.inputType == "tab"))
        throw CLIException("Error. Parameter -f value may be either \"fasta\" or \"tab\" in mode " + mode + ".");
}

// checkCommonArgs, Hammock.java:1212-1232: -d must not exist; without it, dist/Hammock_result_<i> beside the binary
void makeOutputDirectory(Options &o, const std::string &parentDir) {
    if (o.haveDir) {
        if (exists(o.workingDirectory)) throw CLIException("Error. Output directory exists. Exiting to prevent data loss.");
        mkdir(o.workingDirectory.c_str(), 0777);
        return;
    }
    std::string name;
    mkdir((parentDir + "/dist").c_str(), 0777);
    for (int i = 1; i < 9999; i++) {
        name = parentDir + "/dist/Hammock_result_" + std::to_string(i);
        if (!exists(name)) { mkdir(name.c_str(), 0777); break; }
    }
    o.workingDirectory = name;
    std::cerr << "Creating default output directory: " << name << std::endl;
}

// The banner, the matrix (Hammock.java:1264) and the GPU context: HIP start-up, queues and code objects take 70-150 ms, so the
// context is created on another thread while the caller reads and summarises its input.  clustering (greedy, clinkage): over
// --devices when given, with --java_hashset applied; the other modes run on --device alone.
ContextFuture beginRun(const Options &o, const Logger &logger, bool clustering) {
    logger.logAndStderr(std::string("\nHammock version ") + VERSION +
                        " Run with --help for a brief description of command line parameters.\n");
    const std::vector<std::vector<int>> scoringMatrix = FileIOManager::loadScoringMatrix(o.matrixFile);
    const std::vector<int> devices = clustering ? o.devices : std::vector<int>();
    const int javaHashSet = clustering ? o.javaHashSet : 8;
    return std::async(std::launch::async, [scoringMatrix, devices, device = o.device, javaHashSet]() {
        std::shared_ptr<NativeContext> c = devices.empty() ? std::make_shared<NativeContext>(scoringMatrix, device)
                                                           : std::make_shared<NativeContext>(scoringMatrix, devices);
        if (javaHashSet != 8 && hmk_set_java_hashset(c->get(), javaHashSet) != HMK_OK) throw HammockException("hmk_set_java_hashset failed");
        return c;
    });
}

void logRunStart(const Logger &logger, const std::string &mode, const std::vector<std::string> &args) {  // Hammock.java:225-229, :244-248
    logger.logWithTime("Program started in mode \"" + mode + "\".");
    std::string argsString;
    for (auto &a : args) argsString += " " + a;
    logger.logWithoutTime("Command-line arguments: \n" + argsString + "\n");
}

// The catch ladder of a run (Hammock.java:146-167), called from `catch (...)`: logs the exception in flight and returns the exit
// code; a CLIException goes on to main.  Only greedy and clinkage give a NullPointerException the reference's exit code 4 (:153-157).
// Of the other modes' calls hmk_clinkage_merge can return HMK_ERR_REFERENCE_WOULD_CRASH (the chain returns to a cluster on its
// stack); hmk_greedy_continue cannot.  Merge reports it as any other error, 6.
int reportRunError(const Logger &logger, bool clustering) {
    auto other = [&](const std::exception &e) {  // :163-167
        logger.logAndStderr("Error. Run with --help for a brief description of command line parameters. Trace: \n");
        logger.logAndStderr(e.what());
        return 6;
    };
    try {
        throw;
    } catch (const CLIException &) {
        throw;
    } catch (const FileFormatException &e) {  // :148-152
        logger.logAndStderr("Error. Probably wrong input file format? Run with --help for a brief description of command line parameters. Trace: \n");
        logger.logAndStderr(std::string("cz.krejciadam.hammock.FileFormatException: ") + e.what());
        return 3;
    } catch (const NullPointerException &e) {  // :153-157
        if (!clustering) return other(e);
        logger.logAndStderr("Error. Maybe wrong input file format? Run with --help for a brief description of command line parameters. Trace: \n");
        logger.logAndStderr(std::string("java.lang.NullPointerException: ") + e.what());
        return 4;
    } catch (const DataException &e) {  // :158-162
        logger.logAndStderr("Error. Maybe wrong input file format or wrong set of labels? Run with --help for a brief description of command line parameters. Trace: \n");
        logger.logAndStderr(std::string("cz.krejciadam.hammock.DataException: ") + e.what());
        return 5;
    } catch (const std::exception &e) {
        return other(e);
    }
}

// Hammock.java:803-811 after a limit the reference does not have.  clamp: the list whose longest sequence must fit the kernels and
// whose shortest one bounds the shift; mean: the list whose mean length sets the default.
void requireKernelLengths(const SequenceListSummary &clamp) {
    if (clamp.maxLength > HMK_MAX_LEN)   // say so here instead of failing inside the clusterer
        throw HammockException("Error. The longest sequence has " + std::to_string(clamp.maxLength) + " amino acids; the GPU kernels of hammock-hip "
                               "take sequences of up to " + std::to_string(HMK_MAX_LEN) + " (Hammock's domain is 7-20).");
}

void settleMaxShift(Options &o, const Logger &logger, const SequenceListSummary &clamp, const SequenceListSummary &mean, const std::string &note) {
    requireKernelLengths(clamp);
    if (!o.haveMaxShift) {
        o.maxShift = checkMaxShift(clamp, (int)javaRound(mean.meanLength() / 4));
        logger.logAndStderr("Max shift not set. Setting automatically to: " + std::to_string(o.maxShift) + note);
        return;
    }
    const int correct = checkMaxShift(clamp, o.maxShift);
    if (o.maxShift != correct) {
        o.maxShift = correct;
        logger.logAndStderr("Setting max shift to " + std::to_string(correct) +
                            " as the length of the shortest sequence is only " + std::to_string(correct + 1));
    }
}

void settleThreshold(Options &o, const Logger &logger, const SequenceListSummary &mean, const std::string &word, const std::string &note) {  // :394-397 / :452-455
    if (o.haveThreshold) return;
    o.sequenceClusteringThreshold = (int)javaRound(mean.meanLength() * 1.7);
    logger.logAndStderr(word + " threshold not set. Setting automatically to: " + std::to_string(o.sequenceClusteringThreshold) + note);
}

// the newer modes settle all three at once (greedy and clinkage write their statistics file between the first two and have the
// reference's silent -p 0); only search takes its two means from different lists
void settleShiftAndThreshold(Options &o, const Logger &logger, const SequenceListSummary &clamp, const SequenceListSummary &shiftMean,
                             const SequenceListSummary &thresholdMean, const std::string &thresholdWord, const std::string &note = "") {
    settleMaxShift(o, logger, clamp, shiftMean, note);
    settleThreshold(o, logger, thresholdMean, thresholdWord, note);
    if (!o.havePenalty) logger.logAndStderr("Gap penalty not set. Setting automatically to: " + std::to_string(o.shiftPenalty));
}

std::vector<UniqueSequencePtr> loadSequences(const Options &o, const std::string &file) {  // loadInputSequences, :749-762 ("seq" is checked before)
    return o.inputType == "fasta" ? FileIOManager::loadUniqueSequencesFromFasta(file) : FileIOManager::loadUniqueSequencesFromTable(file);
}

std::vector<UniqueSequencePtr> filterSequencesForLabels(const std::vector<UniqueSequencePtr> &sequences, const std::vector<std::string> &labels) {  // :1661-1675
    std::vector<UniqueSequencePtr> kept;
    for (auto &s : sequences) {
        std::vector<std::pair<std::string, int>> lm;
        for (auto &label : labels) {
            bool present = false;
            const int c = s->labelCount(label, &present);
            if (present) lm.push_back({label, c});
        }
        if (!lm.empty()) kept.push_back(std::make_shared<UniqueSequence>(s->getSequenceString(), lm));
    }
    return kept;
}

std::vector<UniqueSequencePtr> sequencesOf(const std::vector<ClusterPtr> &clusters) {
    std::vector<UniqueSequencePtr> sequences;
    for (auto &cl : clusters) for (auto &s : cl->getSequences()) sequences.push_back(s);
    return sequences;
}

void requireOccurrences(const std::vector<UniqueSequencePtr> &sequences, const std::string &where) {
    for (auto &s : sequences)
        if (s->size() < 1) throw FileFormatException(where + " - the sequence " + s->getSequenceString() + " has no occurrences (Cluster.size() counts them).");
}

// The candidate clusters of a list (--skip_singletons: those of more than one unique sequence, LimitedGreedySequenceClusterer.java:41-48)
// as the library takes them: their members appended to `upload`, each member's candidate number, each candidate's id.
struct Candidates {
    std::vector<uint32_t> slots;           // indices into the cluster list
    std::vector<uint32_t> memberCluster;   // per appended member: its candidate
    std::vector<int32_t> clusterId;        // per candidate: getId() + idShift
};
Candidates appendCandidates(const std::vector<ClusterPtr> &clusters, bool skipSingletons, int idShift, std::vector<UniqueSequencePtr> &upload) {
    Candidates cand;
    for (uint32_t c = 0; c < (uint32_t)clusters.size(); c++) {
        if (skipSingletons && clusters[c]->getUniqueSize() <= 1) continue;
        cand.clusterId.push_back(clusters[c]->getId() + idShift);
        for (auto &s : clusters[c]->getSequences()) { upload.push_back(s); cand.memberCluster.push_back((uint32_t)cand.slots.size()); }
        cand.slots.push_back(c);
    }
    return cand;
}

// assignments.tsv and cluster_matches.tsv: per row its best feasible candidates by rank, or one NA line
void writeRankedTable(const std::string &file, const std::string &header, const std::vector<std::string> &rows, const std::vector<ClusterPtr> &clusters,
                      const Candidates &cand, uint32_t best, const std::vector<uint32_t> &bestCluster, const std::vector<int32_t> &bestScore,
                      const std::vector<uint32_t> &nFeasible) {
    std::ofstream out(file);
    if (!out) throw HammockException("cannot write " + file);
    out << header << '\n';
    for (size_t q = 0; q < rows.size(); q++) {
        if (nFeasible[q] == 0) { out << rows[q] << "\tNA\tNA\tNA\tNA\t0\n"; continue; }
        for (uint32_t t = 0; t < std::min(nFeasible[q], best); t++) {
            const ClusterPtr &cl = clusters[cand.slots[bestCluster[q * best + t]]];
            out << rows[q] << '\t' << t + 1 << '\t' << cl->getId() << '\t' << bestScore[q * best + t] << '\t' << cl->size() << '\t' << nFeasible[q] << '\n';
        }
    }
}

// greedy mode (Hammock.java:217-234, runGreedyClustering :392-437) and clinkage mode (:236-253, runClinkageClustering
// :449-489): the two share everything but the clusterer, the ordering step and a few log lines
int runSequenceClustering(const std::vector<std::string> &args, bool clinkage) {
    Options o;
    parseCommonArgs(args, o);
    if (clinkage) parseClinkageArgs(args, o);
    else {
        parseGreedyArgs(args, o);
        parseScorerArgs(args, o);
        if (o.alignments) throw CLIException("Error. --alignments belongs to mode search.");
    }
    requireInput(o);
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, true);
        std::vector<std::string> labels;
        if (o.haveLabels) labels = FileIOManager::splitChar(o.labelString, ',', true);
        const std::string initialClustersSequencesCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string initialClustersSequencesOrderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string initialClusters = o.workingDirectory + "/initial_clusters.tsv";
        const std::string inputStatistics = o.workingDirectory + "/input_statistics.tsv";
        // ---- checkGreedyOrClinkageArgs, :1272-1277 ------------------------------------------------
        if (!(o.inputType == "fasta" || o.inputType == "seq" || o.inputType == "tab"))
            throw CLIException("Error. Parameter -f value may be either \"fasta\", \"seq\" or \"tab\". No other values are allowed");

        logRunStart(logger, clinkage ? "clinkage" : "greedy", args);
        logger.logWithoutTime("\nComplete list of input/output parameters: \n-i, --input " + o.inputFileName +
                              "\n-d, --output_directory " + o.workingDirectory + "\n-t, --thread " + std::to_string(o.nThreads) +
                              "\n-l, --labels " + labelsToString(o.haveLabels, labels) + "\n\n");
        if (clinkage)   // logClinkageParams, :1742-1755 (labels as the reference prints them)
            logger.logWithoutTime("\nComplete list of clinkage clustering parameters: \n-f, --file_format " + o.inputType +
                                  "\n-m, --matrix " + o.matrixFile + "\n-g, --alignment_threshold (--greedy_threshold)" +
                                  (o.haveThreshold ? std::to_string(o.sequenceClusteringThreshold) : std::string("null")) +
                                  "\n-x, --max_shift " + (o.haveMaxShift ? std::to_string(o.maxShift) : std::string("null")) +
                                  "\n-p, --gap_penalty " + std::to_string(o.shiftPenalty) + "\n-C, --cache_size_limit " +
                                  std::to_string(o.cacheSizeLimit) + "\n\n");
        else
        logger.logWithoutTime("\nComplete list of greedy clustering parameters: \n-f, --file_format " + o.inputType +
                              "\n-m, --matrix " + o.matrixFile + "\n-g, --greedy_threshold " +
                              (o.haveThreshold ? std::to_string(o.sequenceClusteringThreshold) : std::string("null")) +
                              "\n-x, --max_shift " + (o.haveMaxShift ? std::to_string(o.maxShift) : std::string("null")) +
                              "\n-p, --gap_penalty " + std::to_string(o.shiftPenalty) + "\n-R, --order " + o.order +
                              "\n-S, --seed " + std::to_string(o.seed) +
                              (o.haveScorer ? std::string("\n--scorer ") + (o.globalScorer ? "global" : "shifted") + "\n--gap_open " +
                                                  std::to_string(o.gapOpen) + "\n--gap_extend " + std::to_string(o.gapExtend)
                                            : std::string()) +
                              "\n\n");

        // ---- loadInputSequences, :749-787 -----------------------------------------------------------
        const auto timeStart = std::chrono::steady_clock::now();
        auto cliLap = [timeStart](const char *what) {   // HMK_CLI_TIMING=1: where a hammock-hip process spends its time
            if (std::getenv("HMK_CLI_TIMING"))
                std::fprintf(stderr, "[hammock-hip] %s at %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - timeStart).count());
        };
        logger.logAndStderr("Loading input sequences...");
        if (o.inputType == "seq") throw HammockException("Error, this should have been checked.");  // :759-761
        std::vector<UniqueSequencePtr> sequences = loadSequences(o, o.inputFileName);
        cliLap("input loaded");
        logger.logAndStderr(std::to_string(sequences.size()) + " unique sequences loaded.");
        SequenceListSummary summary = summariseSequences(sequences);
        logger.logAndStderr(std::to_string(summary.total) + " total sequences loaded.");
        if (o.haveLabels) {
            sequences = filterSequencesForLabels(sequences, labels);
            summary = summariseSequences(sequences);
        }
        logger.logAndStderr(std::to_string(sequences.size()) + " unique sequences after non-specified labels filtered out");
        logger.logAndStderr(std::to_string(summary.total) + " total sequences after non-specified labels fileterd out");
        logger.logAndStderr("Shortest sequence: " + std::to_string(summary.minLength) + " AA. Longest sequence: " + std::to_string(summary.maxLength) + " AA.");
        if (sequences.empty()) throw FileFormatException("Error. No sequences (with specified labels) to cluster.");
        // the sequence count is known: the context's buffers (24 GB at 10^6) are sized on another thread while this one goes on
        // to the labels, the statistics, the sort and the upload
        std::future<void> reserved = std::async(std::launch::async, [contextReady, cliLap, count = (uint32_t)sequences.size(), global = o.globalScorer]() {
            try {   // (a device error is reported by the clustering call)
                if (global) return;   // (hmk_greedy_from_edges merges on the host: nothing to reserve)
                hmk_ctx *c = contextReady.get()->get();
                cliLap("hmk_reserve begins");
                (void)hmk_reserve(c, count);
                cliLap("hmk_reserve done");
            } catch (...) { }
        });

        // ---- runGreedyClustering, :392-437 ------------------------------------------------------------
        if (!o.haveLabels) labels = FileIOManager::getSortedLabels(sequences);                 // :796-798
        const std::vector<UniqueSequencePtr> initialSequences(sequences);                       // :800-801
        if (o.globalScorer) requireKernelLengths(summary);   // (the shift has no part in this scorer)
        else settleMaxShift(o, logger, summary, summary, "");                                   // :803-811
        logScorer(o, logger);
        cliLap("labels, lengths, max shift");
        logger.logAndStderr("Generating input statistics...");
        FileIOManager::saveInputStatistics(sequences, labels, inputStatistics);                 // :814-816
        cliLap("input statistics written");
        settleThreshold(o, logger, summary, clinkage ? "Clinkage clustering" : "Greedy clustering", "");
        if (!clinkage && !o.haveLimit) {                                                                     // :398-401
            o.initialClustersLimit = (int)javaRound((double)sequences.size() * 0.025);
            logger.logAndStderr("Initial greedy clusters limit not set. Setting automatically to: " +
                                std::to_string(o.initialClustersLimit));
        }
        std::shared_ptr<ShiftedScorer> scorer;   // (--scorer global: none)
        if (!o.globalScorer) scorer = std::make_shared<ShiftedScorer>(contextReady.get(), o.shiftPenalty, o.maxShift);  // :402 (get() rethrows a device error)
        HipGreedySequenceClusterer clusterer = o.globalScorer
            ? HipGreedySequenceClusterer(std::make_shared<GlobalAlignmentScorer>(contextReady.get(), o.gapOpen, o.gapExtend),
                                         o.sequenceClusteringThreshold, o.initialClustersLimit)
            : HipGreedySequenceClusterer(scorer, o.sequenceClusteringThreshold, o.initialClustersLimit);  // :403
        HipClinkageSequenceClusterer clinkageClusterer(scorer, o.sequenceClusteringThreshold);                // :459

        cliLap("GPU context ready");
        logger.logAndStderr(clinkage ? "Clinkage clustering..." : "Greedy clustering...");
        const auto time0 = std::chrono::steady_clock::now();
        if (!clinkage) sortSequences(sequences, o.order, o.seed, labels);                       // :407 (clinkage keeps the load order)
        if (std::getenv("HMK_CLI_TIMING"))
            std::fprintf(stderr, "[hammock-hip] sort: %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - time0).count());
        std::vector<ClusterPtr> clusters = clinkage ? clinkageClusterer.cluster(sequences)      // :462
                                                    : clusterer.cluster(sequences);             // :409
        cliLap("clustered");
        logger.logAndStderr("Ready. Clustering time: " + std::to_string(millisSince(time0)));  // :411 / :463
        logger.logAndStderr("Resulting clusers: " + std::to_string(clusters.size()));          // :412 / :464
        if (clinkage)
            logger.logAndStderr("GPU scoring: " + std::to_string(clinkageClusterer.stats.neighbors_ms) + " ms, host nearest-neighbour chain: " +
                                std::to_string(clinkageClusterer.stats.chain_ms) + " ms, neighbour edges: " +
                                std::to_string(clinkageClusterer.stats.n_edges) + ", merges: " + std::to_string(clinkageClusterer.stats.merges));
        else
        logger.logAndStderr("GPU scoring + adjacency build: " + std::to_string(clusterer.stats.neighbors_ms) + " ms, host greedy merge: " +
                            std::to_string(clusterer.stats.greedy_ms) + " ms, neighbour edges: " +
                            std::to_string(clusterer.stats.n_edges));
        logger.logAndStderr("Building MSAs... (skipped: Clustal Omega is outside the scope of hammock-hip; the alignment "
                            "column of multi-member clusters is NA)");
        logger.logAndStderr("Ready. Total time: " + std::to_string(millisSince(time0)));       // :427
        logger.logAndStderr("Saving results to output files...");
        // the reference's three calls in a row (:429, :431, :432), written side by side
        FileIOManager::saveInitialClusters(clusters, initialClustersSequencesCsv, initialClustersSequencesOrderedCsv, initialClusters,
                                           labels, initialSequences);
        cliLap("result files written");
        logger.logAndStderr(std::string(clinkage ? "Clinkage" : "Greedy") + " clustering results in: " + initialClusters);
        logger.logAndStderr("and: " + initialClustersSequencesCsv);
        logger.logAndStderr("and: " + initialClustersSequencesOrderedCsv);
        logger.logWithTime("Program successfully ended.");
        // Everything is on disk (the writers and the logger close their files).  Tearing down 10^6 sequence and cluster
        // objects one by one and handing 36 GB of device buffers back costs 0.3-0.5 s that change nothing: leave at once,
        // the driver reclaims the device memory with the process.  (Handing the
        // context back on another thread while the files are written was measured too: the writers lose 0.1 s to it and the
        // process still needs 0.17 s to go, 1.42-1.51 s against 1.17-1.45 s.)
        cliLap("log closed, leaving");
        std::cout.flush();
        std::cerr.flush();
        std::fflush(nullptr);
        std::_Exit(0);
        return 0;
    } catch (...) {
        return reportRunError(logger, true);
    }
}

// `hammock-hip search -i queries --database references -d dir ...`: every query against every reference with ShiftedScorer
// (sequenceScore(seq1 = query, seq2 = reference)), the hits at or above the threshold to <dir>/search_hits.tsv
// (query, target, score, shift): queries in load order, each one's hits by score descending, then by the reference's load
// order.  Each file is loaded and deduplicated on its own (FileIOManager.loadUniqueSequencesFrom*), so one peptide may be on
// both sides.  Defaults: -x as greedy's over the union of both files (Hammock.java:803-811,1421-1434), -g = round(1.7 x the mean
// query length) (:394-397), -p 0.  --best K: only the best K hits of each query (hmk_search_best_shifted).
// --scorer global: GlobalAlignmentScorer(--gap_open, --gap_extend) through hmk_search_global instead; no -x / -p, the columns are
// query, target, score, and --best K cuts each query's sorted hits to K.  --alignments (with --scorer global only) adds the columns
// query_row and target_row: the gapped alignment of every kept hit (hmk_align_pairs_global, seq1 = query, seq2 = target).
int runSearch(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, 0);
    parseScorerArgs(args, o);
    requireOneDevice(o, "search", "a search");
    requireInput(o);
    if (!o.haveDatabase) throw CLIException("Error. Parameter reference file (--database) missing with no default.");
    requireFastaOrTab(o, "search");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "search", args);
        logger.logAndStderr("Loading query sequences...");
        const std::vector<UniqueSequencePtr> queries = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(queries.size()) + " unique query sequences loaded.");
        logger.logAndStderr("Loading reference sequences...");
        const std::vector<UniqueSequencePtr> references = loadSequences(o, o.database);
        logger.logAndStderr(std::to_string(references.size()) + " unique reference sequences loaded.");
        if (queries.empty() || references.empty()) throw FileFormatException("Error. No sequences to search.");
        std::vector<UniqueSequencePtr> all(queries);
        all.insert(all.end(), references.begin(), references.end());
        const SequenceListSummary summary = summariseSequences(all);
        if (o.globalScorer) {   // (the shift parameters have no part in this scorer)
            requireKernelLengths(summary);
            settleThreshold(o, logger, summariseSequences(queries), "Search", "");
        } else {
            settleShiftAndThreshold(o, logger, summary, summary, summariseSequences(queries), "Search");
        }
        logScorer(o, logger);

        const std::shared_ptr<NativeContext> nc = contextReady.get();
        hmk_ctx *c = nc->get();
        nc->setSequences(all, false);
        const uint32_t nq = (uint32_t)queries.size(), n = (uint32_t)all.size(), best = (uint32_t)o.best;
        logger.logAndStderr("Searching...");
        const auto time0 = std::chrono::steady_clock::now();
        // hits[q] = (score, reference index in load order)
        std::vector<std::vector<std::pair<int, uint32_t>>> hits(nq);
        hmk_neighbor_stats stats{};
        auto byScoreThenReference = [](const std::pair<int, uint32_t> &a, const std::pair<int, uint32_t> &b) {
            return a.first != b.first ? a.first > b.first : a.second < b.second;
        };
        if (o.globalScorer) {   // global(seq1 = query, seq2 = reference); --best K: each query's sorted hits cut to K
            std::vector<uint64_t> edges(1 << 20);
            uint64_t n_edges = 0;
            int st = hmk_search_global(c, 0, nq, nq, n, o.gapOpen, o.gapExtend, o.sequenceClusteringThreshold, edges.data(), edges.size(), &n_edges, &stats);
            if (st == HMK_ERR_CAPACITY) {
                edges.resize(n_edges);
                st = hmk_search_global(c, 0, nq, nq, n, o.gapOpen, o.gapExtend, o.sequenceClusteringThreshold, edges.data(), edges.size(), &n_edges, &stats);
            }
            if (st) nc->raise(st, nullptr);
            for (uint64_t k = 0; k < n_edges; k++)
                hits[HMK_EDGE_M(edges[k])].push_back({HMK_EDGE_SCORE(edges[k]), HMK_EDGE_X(edges[k]) - nq});
            for (auto &h : hits) {
                std::sort(h.begin(), h.end(), byScoreThenReference);
                if (best && h.size() > best) h.resize(best);
            }
        } else if (best) {
            std::vector<uint32_t> index((size_t)nq * best), count(nq);
            std::vector<int32_t> score((size_t)nq * best);
            const int st = hmk_search_best_shifted(c, 0, nq, nq, n, o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold, best,
                                                   index.data(), score.data(), count.data(), &stats);
            if (st) nc->raise(st, nullptr);
            for (uint32_t q = 0; q < nq; q++)
                for (uint32_t t = 0; t < count[q]; t++) hits[q].push_back({score[(size_t)q * best + t], index[(size_t)q * best + t] - nq});
        } else {
            std::vector<uint64_t> edges(1 << 20);
            uint64_t n_edges = 0;
            int st = hmk_search_shifted(c, 0, nq, nq, n, o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold, edges.data(), edges.size(),
                                        &n_edges, &stats);
            if (st == HMK_ERR_CAPACITY) {
                edges.resize(n_edges);
                st = hmk_search_shifted(c, 0, nq, nq, n, o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold, edges.data(), edges.size(),
                                        &n_edges, &stats);
            }
            if (st) nc->raise(st, nullptr);
            for (uint64_t k = 0; k < n_edges; k++)
                hits[HMK_EDGE_M(edges[k])].push_back({HMK_EDGE_SCORE(edges[k]), HMK_EDGE_X(edges[k]) - nq});
            for (auto &h : hits) std::sort(h.begin(), h.end(), byScoreThenReference);
        }
        // AligningScorerResult.getShift() of scoreWithShift(seq1 = query, seq2 = target), for the hits only
        std::vector<uint32_t> pi, pj;
        for (uint32_t q = 0; q < nq; q++)
            for (auto &h : hits[q]) { pi.push_back(q); pj.push_back(nq + h.second); }
        std::vector<int32_t> sc(pi.size()), shift(pi.size());
        if (!pi.empty() && !o.globalScorer) {
            const int st = hmk_score_with_shift(c, pi.data(), pj.data(), pi.size(), o.maxShift, o.shiftPenalty, sc.data(), shift.data());
            if (st) nc->raise(st, nullptr);
        }
        // --alignments: the gapped alignment of every kept hit (seq1 = query, seq2 = target)
        std::vector<GappedAlignment> aligned;
        if (o.alignments && !pi.empty()) {
            aligned = GlobalAlignmentScorer(nc, o.gapOpen, o.gapExtend).alignUploaded(pi, pj);
            size_t k = 0;
            for (uint32_t q = 0; q < nq; q++)
                for (auto &h : hits[q])
                    if (aligned[k++].score != h.first) throw HammockException("an alignment's score differs from its hit's");
        }
        logger.logAndStderr("Ready. Search time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Pairs scored: " + std::to_string(stats.pairs_scored) + ", hits reported: " + std::to_string(pi.size()) +
                            ", GPU kernels: " + std::to_string(stats.kernel_ms) + " ms");
        const std::string hitsFile = o.workingDirectory + "/search_hits.tsv";
        {
            std::ofstream out(hitsFile);
            if (!out) throw HammockException("cannot write " + hitsFile);
            out << (o.alignments ? "query\ttarget\tscore\tquery_row\ttarget_row\n" : o.globalScorer ? "query\ttarget\tscore\n" : "query\ttarget\tscore\tshift\n");
            size_t k = 0;
            for (uint32_t q = 0; q < nq; q++)
                for (auto &h : hits[q]) {
                    out << queries[q]->getSequenceString() << '\t' << references[h.second]->getSequenceString() << '\t' << h.first;
                    if (!o.globalScorer) out << '\t' << shift[k];
                    if (o.alignments) {
                        const auto rows = gappedRows(queries[q]->getSequenceString(), references[h.second]->getSequenceString(), aligned[k]);
                        out << '\t' << rows.first << '\t' << rows.second;
                    }
                    out << '\n';
                    k++;
                }
        }
        logger.logAndStderr("Search results in: " + hitsFile);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip assign -i new.fa --clusters initial_clusters_sequences.tsv -d dir ...`: every new sequence against the clusters of a
// cluster file (FileIOManager.loadClustersFromCsv), complete linkage with ShiftedScorer (sequenceScore(seq1 = member, seq2 = new)),
// the feasible clusters ranked as findNearestClusterParallel ranks them (ClinkageSequenceClusterer.java:243-294; score, then
// size(), then id) to <dir>/assignments.tsv.  The clusters are frozen: new sequences are classified one by one and never see each
// other.  Defaults: -x and -g are greedy's (Hammock.java:394-397, 1421-1434) over the cluster file's sequences, -x then clamped by
// the shortest sequence of both sides (checkMaxShift); -p 0; --best 1.  --skip_singletons: only clusters of more than one unique
// sequence are candidates (LimitedGreedySequenceClusterer.java:41-48).
int runAssign(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, 1);
    requireOneDevice(o, "assign", "an assignment");
    requireInput(o);
    requireClusters(o);
    requireFastaOrTab(o, "assign");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "assign", args);
        logger.logAndStderr("Loading clusters...");
        const std::vector<ClusterPtr> clusters = FileIOManager::loadClustersFromCsv(o.clustersFile);
        const std::vector<UniqueSequencePtr> clusterSequences = sequencesOf(clusters);
        logger.logAndStderr(std::to_string(clusters.size()) + " clusters of " + std::to_string(clusterSequences.size()) + " sequences loaded.");
        logger.logAndStderr("Loading new sequences...");
        const std::vector<UniqueSequencePtr> newSequences = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(newSequences.size()) + " unique new sequences loaded.");
        if (newSequences.empty()) throw FileFormatException("Error. No sequences to assign.");
        if (clusterSequences.empty()) throw FileFormatException("Error. The cluster file holds no clusters.");
        requireOccurrences(clusterSequences, "Error in cluster file: " + o.clustersFile);
        std::vector<UniqueSequencePtr> both(newSequences);
        both.insert(both.end(), clusterSequences.begin(), clusterSequences.end());
        const SequenceListSummary summary = summariseSequences(clusterSequences);
        settleShiftAndThreshold(o, logger, summariseSequences(both), summary, summary, "Assignment");

        // the candidates' members behind the new sequences: new [0, nq), members [nq, n)
        std::vector<UniqueSequencePtr> upload(newSequences);
        const Candidates cand = appendCandidates(clusters, o.skipSingletons, 0, upload);
        const uint32_t nq = (uint32_t)newSequences.size(), n = (uint32_t)upload.size(), best = (uint32_t)o.best;
        const std::shared_ptr<NativeContext> nc = contextReady.get();
        nc->setSequences(upload, true, nq);   // (a new sequence's size plays no part)
        logger.logAndStderr("Assigning...");
        const auto time0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> bestCluster((size_t)nq * best), nFeasible(nq);
        std::vector<int32_t> bestScore((size_t)nq * best);
        hmk_neighbor_stats stats{};
        const int st = hmk_assign_shifted(nc->get(), 0, nq, nq, n, cand.memberCluster.data(), cand.clusterId.data(), (uint32_t)cand.slots.size(),
                                          o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold, best, bestCluster.data(), bestScore.data(),
                                          nFeasible.data(), &stats);
        if (st) nc->raise(st, nullptr);
        const long long ms = millisSince(time0);
        size_t assigned = 0;
        for (uint32_t q = 0; q < nq; q++) assigned += nFeasible[q] > 0;
        logger.logAndStderr("Ready. Assignment time: " + std::to_string(ms));
        logger.logAndStderr("Candidate clusters: " + std::to_string(cand.slots.size()) + ", sequences assigned: " + std::to_string(assigned) + " of " +
                            std::to_string(nq) + ", pairs scored: " + std::to_string(stats.pairs_scored) + ", GPU kernels: " +
                            std::to_string(stats.kernel_ms) + " ms");
        const std::string outFile = o.workingDirectory + "/assignments.tsv";
        std::vector<std::string> rows;
        for (auto &s : newSequences) rows.push_back(s->getSequenceString());
        writeRankedTable(outFile, "sequence\trank\tcluster_id\tscore\tcluster_size\tfeasible_clusters", rows, clusters, cand, best, bestCluster,
                         bestScore, nFeasible);
        logger.logAndStderr("Assignments in: " + outFile);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip match -i query_clusters.tsv --clusters clusters.tsv -d dir ...`: every cluster of the -i cluster file (singletons
// included) against the clusters of the --clusters file, complete linkage over both clusters' members with ShiftedScorer
// (ClinkageClusterScorer.clusterScore(existing, query cluster): seq1 = existing member), the feasible clusters ranked as
// findNearestClusterParallel ranks them (score, then size(), then id) to <dir>/cluster_matches.tsv, in the -i file's cluster order.
// A match means the union of the two clusters is still a complete-linkage cluster; query clusters are matched one by one and
// never checked against each other.  Defaults are assign's: -x and -g are greedy's over the --clusters file's sequences, -x then
// clamped by the shortest sequence of both files; -p 0; --best 1.  --skip_singletons: only --clusters clusters of more than one
// unique sequence are candidates.
int runMatch(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, 1);
    requireOneDevice(o, "match", "a match");
    requireInput(o);
    requireClusters(o);
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "match", args);
        logger.logAndStderr("Loading clusters...");
        const std::vector<ClusterPtr> clusters = FileIOManager::loadClustersFromCsv(o.clustersFile);
        const std::vector<UniqueSequencePtr> clusterSequences = sequencesOf(clusters);
        logger.logAndStderr(std::to_string(clusters.size()) + " clusters of " + std::to_string(clusterSequences.size()) + " sequences loaded.");
        logger.logAndStderr("Loading query clusters...");
        const std::vector<ClusterPtr> queries = FileIOManager::loadClustersFromCsv(o.inputFileName);
        const std::vector<UniqueSequencePtr> querySequences = sequencesOf(queries);
        logger.logAndStderr(std::to_string(queries.size()) + " query clusters of " + std::to_string(querySequences.size()) + " sequences loaded.");
        if (querySequences.empty()) throw FileFormatException("Error. No query clusters to match.");
        if (clusterSequences.empty()) throw FileFormatException("Error. The cluster file holds no clusters.");
        requireOccurrences(clusterSequences, "Error in cluster file: " + o.clustersFile);
        std::vector<UniqueSequencePtr> both(querySequences);
        both.insert(both.end(), clusterSequences.begin(), clusterSequences.end());
        const SequenceListSummary summary = summariseSequences(clusterSequences);
        settleShiftAndThreshold(o, logger, summariseSequences(both), summary, summary, "Match");

        // the query clusters' sequences, then the candidates' members: queries [0, nq), members [nq, n)
        std::vector<UniqueSequencePtr> upload(querySequences);
        std::vector<uint32_t> queryCluster;
        for (uint32_t b = 0; b < (uint32_t)queries.size(); b++) queryCluster.insert(queryCluster.end(), queries[b]->getSequences().size(), b);
        const Candidates cand = appendCandidates(clusters, o.skipSingletons, 0, upload);
        const uint32_t nq = (uint32_t)querySequences.size(), nb = (uint32_t)queries.size(), n = (uint32_t)upload.size(), best = (uint32_t)o.best;
        const std::shared_ptr<NativeContext> nc = contextReady.get();
        nc->setSequences(upload, true, nq);   // (a query sequence's size plays no part)
        logger.logAndStderr("Matching...");
        const auto time0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> bestCluster((size_t)nb * best), nFeasible(nb);
        std::vector<int32_t> bestScore((size_t)nb * best);
        hmk_neighbor_stats stats{};
        const int st = hmk_match_clusters_shifted(nc->get(), 0, nq, queryCluster.data(), nb, nq, n, cand.memberCluster.data(), cand.clusterId.data(),
                                                  (uint32_t)cand.slots.size(), o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold, best,
                                                  bestCluster.data(), bestScore.data(), nFeasible.data(), &stats);
        if (st) nc->raise(st, nullptr);
        const long long ms = millisSince(time0);
        size_t matched = 0;
        for (uint32_t b = 0; b < nb; b++) matched += nFeasible[b] > 0;
        logger.logAndStderr("Ready. Match time: " + std::to_string(ms));
        logger.logAndStderr("Candidate clusters: " + std::to_string(cand.slots.size()) + ", query clusters matched: " + std::to_string(matched) + " of " +
                            std::to_string(nb) + ", pairs scored: " + std::to_string(stats.pairs_scored) + ", GPU kernels: " +
                            std::to_string(stats.kernel_ms) + " ms");
        const std::string outFile = o.workingDirectory + "/cluster_matches.tsv";
        std::vector<std::string> rows;
        for (auto &cl : queries) rows.push_back(std::to_string(cl->getId()));
        writeRankedTable(outFile, "cluster_id\trank\tmatched_cluster_id\tscore\tmatched_size\tfeasible_clusters", rows, clusters, cand, best,
                         bestCluster, bestScore, nFeasible);
        logger.logAndStderr("Matches in: " + outFile);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip continue -i new.fa --clusters initial_clusters_sequences.tsv -d dir ...`: continues the greedy clustering of a cluster
// file with new sequences -- the second loop of LimitedGreedySequenceClusterer.cluster (LimitedGreedySequenceClusterer.java:59-67,
// hmk_greedy_continue) with the file's clusters of more than one unique sequence as actualClusters (:41-50) and the new sequences,
// ordered by -R as greedy orders its input (sortSequences), as actualSequences.  A new sequence that joins a cluster is a member for
// every later one; one that joins nothing is a singleton with id max(loaded id) + 1 + k, k counting them in processing order.
// Phase 1 does not run: new sequences never seed clusters.  The file's singletons are neither candidates nor leftovers.  A new
// sequence already in the file adds its counts and labels to that line's sequence instead.  Defaults: -x and -g are greedy's over
// the file's sequences (they should be the original run's), -x then clamped by the shortest sequence of both sides; -p 0.  Writes
// the stage-1 files of greedy (label columns: the file's, then new labels in first-seen order) and new_sequences.tsv.
int runContinue(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    requireOneDevice(o, "continue", "a continuation");
    requireInput(o);
    requireClusters(o);
    requireFastaOrTab(o, "continue");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "continue", args);
        logger.logAndStderr("Loading clusters...");
        std::vector<ClusterPtr> loaded = FileIOManager::loadClustersFromCsv(o.clustersFile);
        // the file's label columns and its line order (the original-order file lists the file's sequences first, as they came)
        std::vector<std::string> labels;
        std::vector<UniqueSequencePtr> lineOrder;
        std::unordered_map<std::string, UniqueSequencePtr> inFile;
        for (auto &cl : loaded) for (auto &s : cl->getSequences()) inFile.emplace(s->getSequenceString(), s);
        {
            const std::vector<std::string> lines = FileIOManager::readLines(o.clustersFile);
            std::vector<std::string> header = FileIOManager::splitChar(lines[0], CSV_SEPARATOR, true);
            const long seqAt = 1;   // (files greedy writes: cluster_id, sequence, labels...)
            for (const char *drop : {"alignment", "sum"}) {
                const auto at = std::find(header.begin(), header.end(), drop);
                if (at != header.end()) header.erase(at);
            }
            labels.assign(header.begin() + 2, header.end());
            for (size_t k = 1; k < lines.size(); k++) {
                const std::vector<std::string> f = FileIOManager::splitChar(lines[k], CSV_SEPARATOR, true);
                if ((long)f.size() <= seqAt) continue;
                const auto it = inFile.find(f[seqAt]);
                if (it != inFile.end()) lineOrder.push_back(it->second);
            }
        }
        if (o.haveLabels) labels = FileIOManager::splitChar(o.labelString, ',', true);
        const size_t nLoadedSeqs = sequencesOf(loaded).size();
        logger.logAndStderr(std::to_string(loaded.size()) + " clusters of " + std::to_string(nLoadedSeqs) + " sequences loaded.");
        logger.logAndStderr("Loading new sequences...");
        std::vector<UniqueSequencePtr> input = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(input.size()) + " unique new sequences loaded.");
        if (input.empty()) throw FileFormatException("Error. No new sequences.");
        if (nLoadedSeqs == 0) throw FileFormatException("Error. The cluster file holds no clusters.");
        // new labels after the file's, in first-seen order
        if (!o.haveLabels)
            for (auto &s : input)
                for (auto &e : s->getLabelsMap())
                    if (std::find(labels.begin(), labels.end(), e.first) == labels.end()) labels.push_back(e.first);
        // a new sequence already in the file: its counts and labels go to that sequence, which then is not new
        std::vector<UniqueSequencePtr> newSequences;
        size_t merged = 0;
        for (auto &s : input) {
            const auto it = inFile.find(s->getSequenceString());
            if (it == inFile.end()) { newSequences.push_back(s); continue; }
            for (auto &e : s->getLabelsMap()) it->second->addLabelCount(e.first, e.second);
            merged++;
        }
        logger.logAndStderr(std::to_string(merged) + " new sequences were already in the cluster file: their counts and labels were added there.");
        // (Cluster.size() sums its sequences' sizes when it is made: made again after the merge)
        std::vector<ClusterPtr> clusters;
        int maxId = INT32_MIN;
        for (auto &cl : loaded) { clusters.push_back(std::make_shared<Cluster>(cl->getSequences(), cl->getId())); maxId = std::max(maxId, cl->getId()); }
        const std::vector<UniqueSequencePtr> fileSequences = sequencesOf(clusters);
        std::vector<UniqueSequencePtr> both(fileSequences);
        both.insert(both.end(), newSequences.begin(), newSequences.end());
        const SequenceListSummary summary = summariseSequences(fileSequences);
        settleShiftAndThreshold(o, logger, summariseSequences(both), summary, summary, "Greedy clustering", " (it should be the original run's)");
        sortSequences(newSequences, o.order, o.seed, labels);                                    // :407, as greedy orders its input

        // the candidates' members first, the new sequences behind them: members [0, nm), new [nm, n)
        std::vector<UniqueSequencePtr> upload;
        const Candidates cand = appendCandidates(clusters, true, 0, upload);                     // :41-50
        const uint32_t nm = (uint32_t)upload.size(), nq = (uint32_t)newSequences.size();
        upload.insert(upload.end(), newSequences.begin(), newSequences.end());
        const uint32_t n = (uint32_t)upload.size();
        std::vector<int32_t> joined(nq, -1), rank(nq, -1);
        hmk_continue_stats stats{};
        logger.logAndStderr("Continuing the clustering...");
        const auto time0 = std::chrono::steady_clock::now();
        if (nq) {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(upload, true);
            const int st = hmk_greedy_continue(nc->get(), nm, n, 0, nm, cand.memberCluster.data(), cand.clusterId.data(), (uint32_t)cand.slots.size(),
                                               o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold, joined.data(), rank.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        // :61-62 in loop order, then :64-67: the new singletons behind the loaded clusters
        std::vector<ClusterPtr> result(clusters);
        std::vector<int32_t> finalId(nq);
        int k = 0;
        for (uint32_t q = 0; q < nq; q++) {
            if (joined[q] >= 0) {
                const ClusterPtr &cl = clusters[cand.slots[joined[q]]];
                cl->insert(newSequences[q]);
                finalId[q] = cl->getId();
            } else {
                finalId[q] = maxId + 1 + k++;
                result.push_back(std::make_shared<Cluster>(std::vector<UniqueSequencePtr>{newSequences[q]}, finalId[q]));
            }
        }
        logger.logAndStderr("Ready. Clustering time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Candidate clusters: " + std::to_string(cand.slots.size()) + ", new sequences joined: " + std::to_string(stats.n_joined) +
                            " of " + std::to_string(nq) + ", pairs scored: " + std::to_string(stats.pairs_scored) + ", neighbour edges: " +
                            std::to_string(stats.n_edges) + ", GPU passes: " + std::to_string(stats.kernel_ms) + " ms, loop: " +
                            std::to_string(stats.loop_ms) + " ms in " + std::to_string(stats.loop_rounds) + " rounds");
        logger.logAndStderr("Resulting clusers: " + std::to_string(result.size()));
        logger.logAndStderr("Saving results to output files...");
        std::vector<UniqueSequencePtr> originalOrder(lineOrder);
        for (auto &s : input)
            if (std::find(newSequences.begin(), newSequences.end(), s) != newSequences.end()) originalOrder.push_back(s);
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string orderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string clustersCsv = o.workingDirectory + "/initial_clusters.tsv";
        FileIOManager::saveInitialClusters(result, seqCsv, orderedCsv, clustersCsv, labels, originalOrder);
        const std::string newCsv = o.workingDirectory + "/new_sequences.tsv";
        {
            std::ofstream out(newCsv);
            if (!out) throw HammockException("cannot write " + newCsv);
            out << "sequence\tcluster_id\tjoined\n";
            for (uint32_t q = 0; q < nq; q++) out << newSequences[q]->getSequenceString() << '\t' << finalId[q] << '\t' << (joined[q] >= 0 ? 1 : 0) << '\n';
        }
        logger.logAndStderr("Greedy clustering results in: " + clustersCsv);
        logger.logAndStderr("and: " + seqCsv);
        logger.logAndStderr("and: " + orderedCsv);
        logger.logAndStderr("New sequences in: " + newCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip merge -i clusters.tsv [--clusters other.tsv] -d dir ...`: merges the clusters of one or two cluster files by complete
// linkage -- ClinkageSequenceClusterer.cluster (ClinkageSequenceClusterer.java:43-124) started from the given clusters instead of
// from one cluster per sequence (:50-55; hmk_clinkage_merge).  One file: its clusters are merged among themselves.  With --clusters:
// that file's clusters keep their ids and come first in slot order; the -i file's clusters follow, renumbered
// max(--clusters id) + 1 + k in file order; a sequence present in both files stays in its --clusters cluster, gets the -i line's
// counts and labels added (the rule of continue) and leaves its -i cluster, which disappears when it becomes empty.
// --skip_singletons: clusters of one unique sequence are not candidates and are written through unchanged.  Merged clusters get the
// ids max(every id) + 2, + 3, ... in merge order (:97, counted from the largest id of all the clusters, so that a merged cluster
// never takes the id of a cluster that was written through; a file whose ids start below 1 -- greedy numbers clusters by their
// seed's index, from 0 -- goes to the library with its ids shifted up, which only the HashSet orders see).  Defaults of -x / -g are match's (greedy's over the first file's
// sequences, -x clamped by the shortest sequence of all); -p 0.  Writes the stage-1 files of greedy for the merged clustering
// (label columns: the first file's, then the other's new ones) and merged_clusters.tsv, one line per given cluster in slot order.
struct MergeInput {
    std::vector<ClusterPtr> clusters;          // slot order over both files (ids final: the -i file's renumbered)
    std::vector<int> sourceFile, sourceId;     // per cluster: 0 = --clusters (or the only file), 1 = -i; its id in that file
    std::vector<std::string> labels;
    std::vector<UniqueSequencePtr> lineOrder;  // the files' sequences in line order
    size_t duplicates = 0, emptied = 0;
};

static MergeInput loadMergeInput(const std::string &firstFile, const std::string &secondFile) {
    MergeInput in;
    std::unordered_map<std::string, UniqueSequencePtr> inFirst;
    int maxId = INT32_MIN;
    auto header = [&](const std::string &file, const std::vector<ClusterPtr> &loaded) {
        std::unordered_map<std::string, std::vector<UniqueSequencePtr>> byString;   // (every line is a sequence of its own, duplicates included)
        for (auto &cl : loaded) for (auto &s : cl->getSequences()) byString[s->getSequenceString()].push_back(s);
        const std::vector<std::string> lines = FileIOManager::readLines(file);
        std::vector<std::string> h = FileIOManager::splitChar(lines[0], CSV_SEPARATOR, true);
        for (const char *drop : {"alignment", "sum"}) {
            const auto at = std::find(h.begin(), h.end(), drop);
            if (at != h.end()) h.erase(at);
        }
        for (size_t k = 2; k < h.size(); k++)
            if (std::find(in.labels.begin(), in.labels.end(), h[k]) == in.labels.end()) in.labels.push_back(h[k]);
        std::unordered_map<std::string, size_t> taken;
        for (size_t k = 1; k < lines.size(); k++) {
            const std::vector<std::string> f = FileIOManager::splitChar(lines[k], CSV_SEPARATOR, true);
            if (f.size() < 2) continue;
            const auto it = byString.find(f[1]);
            if (it == byString.end()) continue;
            size_t &t = taken[f[1]];
            if (t < it->second.size()) in.lineOrder.push_back(it->second[t++]);
        }
    };
    const std::vector<ClusterPtr> first = FileIOManager::loadClustersFromCsv(firstFile);
    header(firstFile, first);
    for (auto &cl : first) {
        in.clusters.push_back(cl);
        in.sourceFile.push_back(0);
        in.sourceId.push_back(cl->getId());
        maxId = std::max(maxId, cl->getId());
        for (auto &s : cl->getSequences()) inFirst.emplace(s->getSequenceString(), s);
    }
    if (secondFile.empty()) return in;
    const std::vector<ClusterPtr> second = FileIOManager::loadClustersFromCsv(secondFile);
    const size_t firstLines = in.lineOrder.size();
    header(secondFile, second);
    std::unordered_set<const UniqueSequence *> dropped;
    int k = 0;
    for (auto &cl : second) {
        std::vector<UniqueSequencePtr> kept;
        for (auto &s : cl->getSequences()) {
            const auto it = inFirst.find(s->getSequenceString());
            if (it == inFirst.end()) { kept.push_back(s); continue; }
            for (auto &e : s->getLabelsMap()) it->second->addLabelCount(e.first, e.second);
            dropped.insert(s.get());
            in.duplicates++;
        }
        const int id = maxId + 1 + k++;
        if (kept.empty()) { in.emptied++; continue; }
        in.clusters.push_back(std::make_shared<Cluster>(kept, id));
        in.sourceFile.push_back(1);
        in.sourceId.push_back(cl->getId());
    }
    in.lineOrder.erase(std::remove_if(in.lineOrder.begin() + firstLines, in.lineOrder.end(),
                                      [&](const UniqueSequencePtr &s) { return dropped.count(s.get()) != 0; }), in.lineOrder.end());
    // (Cluster.size() sums its sequences' sizes when it is made: the first file's clusters again, after the counts were added)
    for (size_t c = 0; c < in.clusters.size(); c++)
        if (in.sourceFile[c] == 0) in.clusters[c] = std::make_shared<Cluster>(in.clusters[c]->getSequences(), in.clusters[c]->getId());
    return in;
}

int runMerge(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    requireOneDevice(o, "merge", "a merge");
    requireInput(o);
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "merge", args);
        logger.logAndStderr("Loading clusters...");
        const std::string firstFile = o.clustersFile.empty() ? o.inputFileName : o.clustersFile;
        MergeInput in = loadMergeInput(firstFile, o.clustersFile.empty() ? std::string() : o.inputFileName);
        if (o.haveLabels) in.labels = FileIOManager::splitChar(o.labelString, ',', true);
        const std::vector<UniqueSequencePtr> all = sequencesOf(in.clusters);
        std::vector<UniqueSequencePtr> firstSequences;
        for (size_t c = 0; c < in.clusters.size(); c++)
            if (in.sourceFile[c] == 0) firstSequences.insert(firstSequences.end(), in.clusters[c]->getSequences().begin(), in.clusters[c]->getSequences().end());
        logger.logAndStderr(std::to_string(in.clusters.size()) + " clusters of " + std::to_string(all.size()) + " sequences loaded.");
        if (!o.clustersFile.empty())
            logger.logAndStderr(std::to_string(in.duplicates) + " sequences of the input file were already in the cluster file: their counts and labels "
                                "were added there (" + std::to_string(in.emptied) + " input clusters became empty).");
        if (firstSequences.empty()) throw FileFormatException("Error. The cluster file holds no clusters.");
        requireOccurrences(all, "Error in cluster file");
        const SequenceListSummary summary = summariseSequences(firstSequences);
        settleShiftAndThreshold(o, logger, summariseSequences(all), summary, summary, "Merge");

        // the candidates' members, slot by slot
        int maxId = INT32_MIN, minId = INT32_MAX;
        for (auto &cl : in.clusters) {
            maxId = std::max(maxId, cl->getId());
            minId = std::min(minId, cl->getId());
        }
        // (hmk_clinkage_merge takes ids from 1; greedy numbers its clusters by their seed's index, from 0: such ids go to the library
        // shifted up and come back shifted down)
        const int idShift = minId < 1 ? 1 - minId : 0;
        std::vector<UniqueSequencePtr> upload;
        const Candidates cand = appendCandidates(in.clusters, o.skipSingletons, idShift, upload);
        const uint32_t n = (uint32_t)upload.size(), ncl = (uint32_t)cand.slots.size();
        std::vector<int32_t> mergedId(std::max<uint32_t>(ncl, 1)), resultOrder(std::max<uint32_t>(ncl, 1)), rank(std::max<uint32_t>(n, 1));
        hmk_merge_stats stats{};
        logger.logAndStderr("Merging...");
        const auto time0 = std::chrono::steady_clock::now();
        if (ncl >= 1) {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(upload, true);
            int st = hmk_set_java_hashset(nc->get(), o.javaHashSet);
            if (st) nc->raise(st, nullptr);
            st = hmk_clinkage_merge(nc->get(), 0, n, cand.memberCluster.data(), cand.clusterId.data(), ncl, o.maxShift, o.shiftPenalty,
                                    o.sequenceClusteringThreshold, mergedId.data(), resultOrder.data(), rank.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        const long long ms = millisSince(time0);
        // the returned clusters in list order (:121-123), members in Cluster.getSequences() order (:105-106); then the clusters that
        // were written through.  A merged cluster's id counts from the largest id of ALL clusters.
        int maxCandidateId = INT32_MIN;
        for (int32_t id : cand.clusterId) maxCandidateId = std::max(maxCandidateId, id);
        auto finalIdOf = [&](int32_t id) { return id > maxCandidateId ? id - maxCandidateId + maxId : id - idShift; };
        std::unordered_map<int32_t, std::vector<UniqueSequencePtr>> membersOf;
        std::unordered_map<int32_t, int> sourcesOf;
        for (uint32_t c = 0; c < ncl; c++) sourcesOf[mergedId[c]]++;
        for (uint32_t k = 0; k < n; k++) {
            std::vector<UniqueSequencePtr> &m = membersOf[mergedId[cand.memberCluster[k]]];
            if (m.size() <= (size_t)rank[k]) m.resize((size_t)rank[k] + 1);
            m[rank[k]] = upload[k];
        }
        std::vector<ClusterPtr> result;
        for (int32_t t = 0; t < stats.n_result_clusters; t++)
            result.push_back(std::make_shared<Cluster>(membersOf[resultOrder[t]], finalIdOf(resultOrder[t])));
        std::vector<int32_t> slotOf(in.clusters.size(), -1);
        for (uint32_t c = 0; c < ncl; c++) slotOf[cand.slots[c]] = (int32_t)c;
        for (size_t c = 0; c < in.clusters.size(); c++)
            if (slotOf[c] < 0) result.push_back(in.clusters[c]);
        logger.logAndStderr("Ready. Merge time: " + std::to_string(ms));
        logger.logAndStderr("Candidate clusters: " + std::to_string(ncl) + ", merges: " + std::to_string(stats.merges) + ", feasible cluster pairs: " +
                            std::to_string(stats.cluster_pairs) + ", pairs scored: " + std::to_string(stats.pairs_scored) + ", neighbour edges: " +
                            std::to_string(stats.n_edges) + ", GPU pass: " + std::to_string(stats.kernel_ms) + " ms, cluster graph: " +
                            std::to_string(stats.graph_ms) + " ms, chain: " + std::to_string(stats.chain_ms) + " ms");
        logger.logAndStderr("Resulting clusers: " + std::to_string(result.size()));
        logger.logAndStderr("Saving results to output files...");
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string orderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string clustersCsv = o.workingDirectory + "/initial_clusters.tsv";
        FileIOManager::saveInitialClusters(result, seqCsv, orderedCsv, clustersCsv, in.labels, in.lineOrder);
        const std::string mergedCsv = o.workingDirectory + "/merged_clusters.tsv";
        {
            std::ofstream out(mergedCsv);
            if (!out) throw HammockException("cannot write " + mergedCsv);
            out << "source_file\tsource_cluster_id\tcluster_id\tmerged\n";
            for (size_t c = 0; c < in.clusters.size(); c++) {
                const std::string &file = in.sourceFile[c] == 0 ? firstFile : o.inputFileName;
                if (slotOf[c] < 0) { out << file << '\t' << in.sourceId[c] << '\t' << in.clusters[c]->getId() << "\t0\n"; continue; }
                const int32_t id = mergedId[slotOf[c]];
                out << file << '\t' << in.sourceId[c] << '\t' << finalIdOf(id) << '\t' << (sourcesOf[id] > 1 ? 1 : 0) << '\n';
            }
        }
        logger.logAndStderr("Merged clustering in: " + clustersCsv);
        logger.logAndStderr("and: " + seqCsv);
        logger.logAndStderr("and: " + orderedCsv);
        logger.logAndStderr("Given clusters in: " + mergedCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip check -i clusters.tsv -d dir [-x -p -g] [--skip_singletons]`: is the clustering of a cluster file (the format the
// other modes read through --clusters) a set of complete-linkage clusters at these parameters?  hmk_cluster_linkage_shifted over the
// file's clusters: per cluster the minimum ShiftedScorer score over the pairs of its sequences (ClinkageClusterScorer.java:30-49
// without the early exit, inside one cluster), the pair that attains it and the number of pairs below the threshold; per sequence
// its own minimum and count.  Defaults of -x / -g are greedy's over the file's sequences, -x clamped by the shortest one; -p 0.
// Writes cluster_linkage.tsv (one line per cluster in file order; --skip_singletons leaves clusters of one unique sequence out)
// and cluster_members.tsv (the sequences of clusters of more than one, in file order).  The exit status says whether the run
// succeeded, not what it found; a cluster file the loader rejects is an error of the arguments here, 2.
int runCheck(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    requireOneDevice(o, "check", "a check");
    requireInput(o);
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "check", args);
        logger.logAndStderr("Loading clusters...");
        std::vector<ClusterPtr> clusters;
        try {
            clusters = FileIOManager::loadClustersFromCsv(o.inputFileName);
            if (clusters.empty()) throw FileFormatException("Error. The cluster file holds no clusters.");
        } catch (const FileFormatException &e) {
            logger.logAndStderr("Error. Probably wrong input file format? Run with --help for a brief description of command line parameters. Trace: \n");
            logger.logAndStderr(std::string("cz.krejciadam.hammock.FileFormatException: ") + e.what());
            return 2;
        }
        const std::vector<UniqueSequencePtr> all = sequencesOf(clusters);
        logger.logAndStderr(std::to_string(clusters.size()) + " clusters of " + std::to_string(all.size()) + " sequences loaded.");
        const SequenceListSummary summary = summariseSequences(all);
        settleShiftAndThreshold(o, logger, summary, summary, summary, "Check");

        std::vector<UniqueSequencePtr> upload;
        const Candidates cand = appendCandidates(clusters, false, 0, upload);
        const uint32_t n = (uint32_t)upload.size(), ncl = (uint32_t)cand.slots.size();
        std::vector<int32_t> minScore(ncl), memberMin(n);
        std::vector<uint32_t> minA(ncl), minB(ncl), memberBelow(n);
        std::vector<uint64_t> nBelow(ncl);
        hmk_linkage_stats stats{};
        logger.logAndStderr("Checking...");
        const auto time0 = std::chrono::steady_clock::now();
        {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(upload, true);
            const int st = hmk_cluster_linkage_shifted(nc->get(), 0, n, cand.memberCluster.data(), ncl, o.maxShift, o.shiftPenalty,
                                                       o.sequenceClusteringThreshold, minScore.data(), minA.data(), minB.data(), nBelow.data(),
                                                       memberMin.data(), memberBelow.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        logger.logAndStderr("Ready. Check time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Clusters of more than one sequence: " + std::to_string(stats.n_multi) + ", pairs scored: " + std::to_string(stats.pairs_scored) +
                            ", GPU kernels: " + std::to_string(stats.kernel_ms) + " ms");
        logger.logAndStderr("Saving results to output files...");
        const std::string linkageCsv = o.workingDirectory + "/cluster_linkage.tsv", membersCsv = o.workingDirectory + "/cluster_members.tsv";
        {
            std::ofstream out(linkageCsv);
            if (!out) throw HammockException("cannot write " + linkageCsv);
            out << "cluster_id\tunique_size\tsize\tlinkage_score\tpairs_below\tworst_sequence_1\tworst_sequence_2\n";
            for (uint32_t c = 0; c < ncl; c++) {
                const Cluster &cl = *clusters[c];
                if (cl.getUniqueSize() <= 1) {
                    if (!o.skipSingletons) out << cl.getId() << '\t' << cl.getUniqueSize() << '\t' << cl.size() << "\tNA\t0\tNA\tNA\n";
                    continue;
                }
                out << cl.getId() << '\t' << cl.getUniqueSize() << '\t' << cl.size() << '\t' << minScore[c] << '\t' << nBelow[c] << '\t'
                    << upload[minA[c]]->getSequenceString() << '\t' << upload[minB[c]]->getSequenceString() << '\n';
            }
        }
        {
            std::ofstream out(membersCsv);
            if (!out) throw HammockException("cannot write " + membersCsv);
            out << "cluster_id\tsequence\tmin_score\tpairs_below\n";
            // in the file's line order: the loader groups the lines by cluster, so each line finds its sequence again by (id, string),
            // equal lines in their order
            std::map<std::pair<int, std::string>, std::deque<uint32_t>> uploaded;
            for (uint32_t k = 0; k < n; k++)
                uploaded[{clusters[cand.memberCluster[k]]->getId(), upload[k]->getSequenceString()}].push_back(k);
            const std::vector<std::string> lines = FileIOManager::readLines(o.inputFileName);
            std::vector<std::string> header = FileIOManager::splitChar(lines[0], CSV_SEPARATOR, true);
            std::vector<long> dropped;   // the columns the loader drops, in its order
            for (const char *drop : {"alignment", "sum"}) {
                const auto at = std::find(header.begin(), header.end(), drop);
                if (at == header.end()) continue;
                dropped.push_back((long)(at - header.begin()));
                header.erase(at);
            }
            for (size_t l = 1; l < lines.size(); l++) {
                std::vector<std::string> f = FileIOManager::splitChar(lines[l], CSV_SEPARATOR, true);
                for (long d : dropped) f.erase(f.begin() + d);
                std::deque<uint32_t> &q = uploaded.at({javaIntegerDecode(f[0]), f[1]});
                const uint32_t k = q.front();
                q.pop_front();
                const Cluster &cl = *clusters[cand.memberCluster[k]];
                if (cl.getUniqueSize() <= 1) continue;
                out << cl.getId() << '\t' << upload[k]->getSequenceString() << '\t' << memberMin[k] << '\t' << memberBelow[k] << '\n';
            }
        }
        logger.logAndStderr("Clusters in: " + linkageCsv);
        logger.logAndStderr("Sequences in: " + membersCsv);
        std::string lowest = "NA";
        {
            int32_t best = INT32_MAX;
            for (uint32_t c = 0; c < ncl; c++)
                if (clusters[c]->getUniqueSize() > 1 && minScore[c] < best) {
                    best = minScore[c];
                    lowest = std::to_string(best) + " (cluster " + std::to_string(clusters[c]->getId()) + ")";
                }
        }
        logger.logAndStderr(std::to_string(stats.n_violating) + " of " + std::to_string(ncl) + " clusters hold a pair below the threshold " +
                            std::to_string(o.sequenceClusteringThreshold) + "; lowest linkage score " + lowest);
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip split -i clusters.tsv -d dir [-x -p -g] [--java_hashset V]`: splits the clusters of a cluster file into complete-linkage
// clusters at these parameters -- what acts on check's answer.  hmk_clinkage_split over the file's clusters: per cluster
// ClinkageSequenceClusterer.cluster (ClinkageSequenceClusterer.java:43-124) on its sequences alone, in file order.  Defaults of
// -x / -g / -p are check's.  The result list is the source clusters in file order: a cluster that comes back in one part is written as
// it was read (same id, same member order); the parts of a split cluster follow in list order (:121-123), their members in
// getSequences() order (:105-106), their ids continuing from the file's largest id in that order.  Writes the stage-1 files of greedy
// and split_clusters.tsv, one line per resulting cluster.  Exit codes as check: a cluster file the loader rejects is 2.
int runSplit(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    requireOneDevice(o, "split", "a split");
    requireInput(o);
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "split", args);
        logger.logAndStderr("Loading clusters...");
        MergeInput in;
        try {
            in = loadMergeInput(o.inputFileName, std::string());
            if (in.clusters.empty()) throw FileFormatException("Error. The cluster file holds no clusters.");
        } catch (const FileFormatException &e) {
            logger.logAndStderr("Error. Probably wrong input file format? Run with --help for a brief description of command line parameters. Trace: \n");
            logger.logAndStderr(std::string("cz.krejciadam.hammock.FileFormatException: ") + e.what());
            return 2;
        }
        const std::vector<ClusterPtr> &clusters = in.clusters;
        if (o.haveLabels) in.labels = FileIOManager::splitChar(o.labelString, ',', true);
        const std::vector<UniqueSequencePtr> all = sequencesOf(clusters);
        logger.logAndStderr(std::to_string(clusters.size()) + " clusters of " + std::to_string(all.size()) + " sequences loaded.");
        requireOccurrences(all, "Error in cluster file");
        const SequenceListSummary summary = summariseSequences(all);
        settleShiftAndThreshold(o, logger, summary, summary, summary, "Split");
        logger.logAndStderr("Parameters: max shift " + std::to_string(o.maxShift) + ", gap penalty " + std::to_string(o.shiftPenalty) + ", threshold " +
                            std::to_string(o.sequenceClusteringThreshold) + ", java_hashset " + std::to_string(o.javaHashSet));

        std::vector<UniqueSequencePtr> upload;
        const Candidates cand = appendCandidates(clusters, false, 0, upload);
        const uint32_t n = (uint32_t)upload.size(), ncl = (uint32_t)cand.slots.size();
        std::vector<uint32_t> splitCluster(n), nParts(ncl), partStart(ncl + 1);
        std::vector<int32_t> partId(n), rank(n), partOrder(n);
        hmk_split_stats stats{};
        logger.logAndStderr("Splitting...");
        const auto time0 = std::chrono::steady_clock::now();
        {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(upload, true);
            int st = hmk_set_java_hashset(nc->get(), o.javaHashSet);
            if (st) nc->raise(st, nullptr);
            st = hmk_clinkage_split(nc->get(), 0, n, cand.memberCluster.data(), ncl, o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold,
                                    splitCluster.data(), nParts.data(), partId.data(), rank.data(), partOrder.data(), partStart.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        const long long ms = millisSince(time0);
        int maxId = INT32_MIN;
        for (auto &cl : clusters) maxId = std::max(maxId, cl->getId());
        std::vector<ClusterPtr> result;
        std::vector<int> sourceOf, partsOf;   // per resulting cluster: its source cluster's id, that cluster's number of parts
        for (uint32_t c = 0; c < ncl; c++) {   // (every cluster is a candidate: slot c is cluster c, its members upload[partStart[c] ...))
            if (nParts[c] <= 1) {
                result.push_back(clusters[c]);
                sourceOf.push_back(clusters[c]->getId());
                partsOf.push_back(1);
                continue;
            }
            for (uint32_t t = 0; t < nParts[c]; t++) {
                const int32_t id = partOrder[partStart[c] + t];
                std::vector<UniqueSequencePtr> members;
                for (uint32_t k = partStart[c]; k < partStart[c + 1]; k++) {
                    if (partId[k] != id) continue;
                    if (members.size() <= (size_t)rank[k]) members.resize((size_t)rank[k] + 1);
                    members[rank[k]] = upload[k];
                }
                result.push_back(std::make_shared<Cluster>(members, ++maxId));
                sourceOf.push_back(clusters[c]->getId());
                partsOf.push_back((int)nParts[c]);
            }
        }
        logger.logAndStderr("Ready. Split time: " + std::to_string(ms));
        logger.logAndStderr("Clusters of more than one sequence: " + std::to_string(stats.n_multi) + ", pairs scored: " + std::to_string(stats.pairs_scored) +
                            ", pairs at or above the threshold: " + std::to_string(stats.n_edges) + ", merges: " + std::to_string(stats.merges) +
                            ", GPU kernels: " + std::to_string(stats.kernel_ms) + " ms, chains: " + std::to_string(stats.chain_ms) + " ms");
        logger.logAndStderr("Clusters split: " + std::to_string(stats.n_split));
        logger.logAndStderr("Resulting clusers: " + std::to_string(result.size()));
        logger.logAndStderr("Saving results to output files...");
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string orderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string clustersCsv = o.workingDirectory + "/initial_clusters.tsv";
        FileIOManager::saveInitialClusters(result, seqCsv, orderedCsv, clustersCsv, in.labels, in.lineOrder);
        const std::string splitCsv = o.workingDirectory + "/split_clusters.tsv";
        {
            std::ofstream out(splitCsv);
            if (!out) throw HammockException("cannot write " + splitCsv);
            out << "source_cluster_id\tcluster_id\tunique_size\tsize\tparts\n";
            for (size_t k = 0; k < result.size(); k++)
                out << sourceOf[k] << '\t' << result[k]->getId() << '\t' << result[k]->getUniqueSize() << '\t' << result[k]->size() << '\t' << partsOf[k] << '\n';
        }
        logger.logAndStderr("Split clustering in: " + clustersCsv);
        logger.logAndStderr("and: " + seqCsv);
        logger.logAndStderr("and: " + orderedCsv);
        logger.logAndStderr("Resulting clusters by source cluster in: " + splitCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip align -i clusters.tsv -d dir [-x -p -m] [--skip_singletons]`: shows the clusters of a cluster file -- a centre-star
// alignment of each around its medoid in the ungapped model of ShiftedScorer.scoreWithShift (hmk_cluster_align_shifted).  Not the
// Clustal Omega alignment of the reference (ClustalRunner.java:34-66): no gap ever stands inside a peptide.  Defaults of -x / -p are
// check's (-g is settled as there and logged, but nothing is thresholded).  Writes
//   initial_clusters_sequences.tsv   the input's rows in line order in the format of writeClusterSequencesToCsv
//                                    (FileIOManager.java:594-638), the `alignment` column holding every clustered sequence's aligned
//                                    row (a cluster of one keeps its bare string); every loader drops that column, so the file feeds
//                                    the other modes unchanged
//   alignments_initial/<id>.aln      per cluster of more than one sequence, in the shape the reference reads back
//                                    (FileIOManager.java:761-776, Cluster.java:167-176; the directory's name: Hammock.java:1317):
//                                    records ">id_k", k from 1 in the cluster's member order as loaded, each followed by its row
//   cluster_centers.tsv              cluster_id, size (unique sequences), center (the medoid's string), center_sum, width; clusters
//                                    in file order (--skip_singletons leaves clusters of one unique sequence out)
// Exit codes as check: a cluster file the loader rejects is 2.
// `align --scorer global [--gap_open --gap_extend]` writes the same three files with GAPPED rows (alignGlobal below): the centre by
// the sums of GlobalAlignmentScorer scores, the rows a centre-star merge of the members' global alignments with it; -x and -p are
// errors with it, as in search.  No file of align carries a shift, so no column loses its meaning; `profile` does not take it.
//
// `hammock-hip profile -i clusters.tsv -d dir --frequency_matrix F [--background B] [-k/--min_ic 1.2] [-y/--max_gap_proportion 0.2]
// [-h/--min_conserved_positions n] [-u/--max_inner_gaps 0] [--skip_singletons]` aligns as align does, with the same scorer options,
// then reads the alignments as the reference reads Clustal's (hmk_cluster_profile): it writes what align writes, and in addition
//   cluster_profiles.tsv             cluster_id, size, width, conserved, match_states (a string of M / .), passes, kld_match_mean,
//                                    kld_all_mean; clusters in file order
//   position_profiles.tsv            cluster_id, column (from 1), gaps, ic, flags (bit 0 conserved, bit 1 match state), the 20 counts
//   member_kld.tsv                   cluster_id, sequence, kld_match, kld_all; members in the clusters' member order as loaded
// and logs the two "Final system KLD over ..." lines of Hammock.java:696-697.  Doubles are written with %.17g.  --skip_singletons
// leaves the clusters of one unique sequence out of all three.  -h defaults to what Hammock.java:1448-1452 computes; -u above 0
// allows inner gaps (:1337-1341).  A frequency or background file that cannot be read as such is 2, as a bad cluster file.
struct ProfileOptions {
    std::string frequencyFile, backgroundFile;
    bool haveFrequency = false, haveBackground = false, haveMinConserved = false;
    double minIc = 1.2, maxGapProportion = 0.2;   // Hammock.java: minIc, maxGapProportion
    int minConservedPositions = 0, maxInnerGaps = 0;
};

double parseDoubleArg(const std::string &v) {  // Double.parseDouble(args[i + 1].trim())
    const std::string t = FileIOManager::trim(v);
    size_t used = 0;
    double d = 0;
    try { d = std::stod(t, &used); } catch (const std::exception &) { used = std::string::npos; }
    if (t.empty() || used != t.size()) throw HammockException("NumberFormatException: For input string: \"" + v + "\"");
    return d;
}

ProfileOptions parseProfileArgs(const std::vector<std::string> &args) {  // Hammock.java:1099-1140
    ProfileOptions po;
    for (size_t i = 1; i + 1 < args.size(); i++) {
        const std::string &a = args[i];
        if (a == "--frequency_matrix") { po.frequencyFile = args[++i]; po.haveFrequency = true; }
        else if (a == "--background") { po.backgroundFile = args[++i]; po.haveBackground = true; }
        else if (a == "-k" || a == "--min_ic") po.minIc = parseDoubleArg(args[++i]);
        else if (a == "-y" || a == "--max_gap_proportion") po.maxGapProportion = parseDoubleArg(args[++i]);
        else if (a == "-h" || a == "--min_conserved_positions") { po.minConservedPositions = javaIntegerDecode(FileIOManager::trim(args[++i])); po.haveMinConserved = true; }
        else if (a == "-u" || a == "--max_inner_gaps") po.maxInnerGaps = javaIntegerDecode(args[++i]);
    }
    if (!po.haveFrequency) throw CLIException("Error. Parameter frequency matrix (--frequency_matrix) missing with no default.");
    return po;
}

// A frequency matrix as FileIOManager.loadFrequencyMatrix reads it (FileIOManager.java:90-118) into hmk_profile_params.frequency
// ([row letter j][column letter i], in the alphabet's order) -> the header's letters; then the background, one line of 20 numbers in
// that letter order (0.05 throughout without a file)
void loadProfileTables(const ProfileOptions &po, hmk_profile_params &P) {
    std::vector<int> letters;
    std::vector<std::vector<double>> rows;
    bool haveHeader = false;
    auto numbers = [](const std::vector<std::string> &parts, const std::string &file) {
        std::vector<double> v;
        for (const std::string &s : parts) {
            size_t used = 0;
            double d = 0;
            try { d = std::stod(s, &used); } catch (const std::exception &) { used = std::string::npos; }
            if (used != s.size()) throw FileFormatException("Error in file: " + file + ". \"" + s + "\" is not a number.");
            v.push_back(d);
        }
        return v;
    };
    for (const std::string &raw : FileIOManager::readLines(po.frequencyFile)) {
        if (!raw.empty() && raw[0] == '#') continue;
        const std::vector<std::string> parts = FileIOManager::splitWhitespace(raw);
        if (parts.empty()) continue;
        if (!haveHeader) {
            haveHeader = true;
            for (const std::string &s : parts) {
                const char *f = std::strchr(AMINO_ACIDS, (char)std::toupper((unsigned char)s[0]));
                letters.push_back(f && *f ? (int)(f - AMINO_ACIDS) : 99);
            }
            continue;
        }
        rows.push_back(numbers(parts, po.frequencyFile));
    }
    std::vector<int> sorted = letters;
    std::sort(sorted.begin(), sorted.end());
    bool ok = letters.size() == 20 && rows.size() == 20;
    for (int k = 0; ok && k < 20; k++) ok = sorted[k] == k && rows[k].size() == 20;
    if (!ok)
        throw FileFormatException("Error in frequency matrix file: " + po.frequencyFile + ". A header line naming each of the 20 amino acids once "
                                  "and 20 rows of 20 numbers are expected.");
    for (int j = 0; j < 20; j++)
        for (int i = 0; i < 20; i++) P.frequency[letters[j] * 20 + letters[i]] = rows[j][i];
    for (int k = 0; k < 20; k++) P.background[k] = 0.05;
    if (po.haveBackground) {
        std::vector<std::vector<double>> lines;
        for (const std::string &raw : FileIOManager::readLines(po.backgroundFile)) {
            if (!raw.empty() && raw[0] == '#') continue;
            const std::vector<std::string> parts = FileIOManager::splitWhitespace(raw);
            if (!parts.empty()) lines.push_back(numbers(parts, po.backgroundFile));
        }
        if (lines.size() != 1 || lines[0].size() != 20)
            throw FileFormatException("Error in background file: " + po.backgroundFile + ". One line of 20 numbers is expected.");
        for (int k = 0; k < 20; k++) P.background[letters[k]] = lines[0][k];
    }
}

std::string g17(double v) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// `align --scorer global`: the same files with gapped rows.  Per slot (its members follow each other in `upload`) the centre is the
// member with the largest sum of global(seq1 = the pair's larger index, seq2 = its smaller index) over the slot's other members, the
// smallest index among equal sums (the orientation and tie rule of hmk_cluster_align_shifted); the sums come from
// hmk_score_pairs_global over the enumerated inside pairs, chunk by chunk, added up in int64 here.  Every other member is aligned
// with seq1 = the centre, seq2 = the member (hmk_align_pairs_global), and starRows merges a slot's records into rows of one width.
// A slot of one member is its own row.  The shift / column of the ungapped model have no counterpart: a row IS the placement.
void alignGlobal(const std::shared_ptr<NativeContext> &nc, const Options &o, const std::vector<UniqueSequencePtr> &upload, const Candidates &cand,
                 std::vector<uint32_t> &center, std::vector<int64_t> &centerSum, std::vector<uint32_t> &width,
                 std::unordered_map<const UniqueSequence *, std::string> &rows, hmk_align_stats &stats) {
    const uint32_t n = (uint32_t)upload.size(), ncl = (uint32_t)cand.slots.size();
    std::vector<uint32_t> first(ncl + 1, 0);   // slot c's members: upload[first[c] .. first[c + 1])
    for (uint32_t k = 0; k < n; k++) first[cand.memberCluster[k] + 1]++;
    for (uint32_t c = 0; c < ncl; c++) first[c + 1] += first[c];
    std::vector<int64_t> sum(n, 0);
    constexpr size_t CHUNK = (size_t)1 << 22;
    std::vector<uint32_t> pi, pj;
    std::vector<int32_t> sc;
    auto flush = [&]() {
        if (pi.empty()) return;
        sc.resize(pi.size());
        const int st = hmk_score_pairs_global(nc->get(), pi.data(), pj.data(), pi.size(), o.gapOpen, o.gapExtend, sc.data());
        if (st) nc->raise(st, nullptr);
        stats.kernel_ms += hmk_last_kernel_ms(nc->get());
        stats.launches++;
        for (size_t k = 0; k < pi.size(); k++) { sum[pi[k]] += sc[k]; sum[pj[k]] += sc[k]; }
        stats.pairs_scored += pi.size();
        pi.clear();
        pj.clear();
    };
    for (uint32_t c = 0; c < ncl; c++)
        for (uint32_t b = first[c] + 1; b < first[c + 1]; b++)
            for (uint32_t a = first[c]; a < b; a++) {
                pi.push_back(b);   // seq1 = the larger index
                pj.push_back(a);
                if (pi.size() == CHUNK) flush();
            }
    flush();
    for (uint32_t c = 0; c < ncl; c++) {
        uint32_t z = first[c];
        for (uint32_t k = first[c] + 1; k < first[c + 1]; k++)
            if (sum[k] > sum[z]) z = k;
        center[c] = z;
        centerSum[c] = sum[z];
        for (uint32_t k = first[c]; k < first[c + 1]; k++)
            if (k != z) { pi.push_back(z); pj.push_back(k); }
    }
    const std::vector<GappedAlignment> records = GlobalAlignmentScorer(nc, o.gapOpen, o.gapExtend).alignUploaded(pi, pj);
    if (!pi.empty()) { stats.kernel_ms += hmk_last_kernel_ms(nc->get()); stats.launches++; }
    size_t r = 0;
    for (uint32_t c = 0; c < ncl; c++) {
        const uint32_t s = first[c + 1] - first[c];
        const std::string &z = upload[center[c]]->getSequenceString();
        std::vector<std::string> members;
        for (uint32_t k = first[c]; k < first[c + 1]; k++)
            if (k != center[c]) members.push_back(upload[k]->getSequenceString());
        const auto star = starRows(z, members, std::vector<GappedAlignment>(records.begin() + r, records.begin() + r + members.size()));
        r += members.size();
        size_t t = 0;
        for (uint32_t k = first[c]; k < first[c + 1]; k++) rows.emplace(upload[k].get(), k == center[c] ? star.first : star.second[t++]);
        width[c] = (uint32_t)star.first.size();
        stats.max_width = std::max(stats.max_width, width[c]);
        if (s > 1) stats.n_multi++;
    }
}

int runAlign(const std::vector<std::string> &args, bool profile = false) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    parseScorerArgs(args, o);
    const std::string mode = profile ? "profile" : "align";
    if (profile && o.globalScorer) throw CLIException("Error. --scorer global is not available in mode profile (its rows carry gaps inside peptides; use align).");
    if (o.alignments) throw CLIException("Error. --alignments belongs to mode search.");
    requireOneDevice(o, mode, profile ? "a profile" : "an alignment");
    requireInput(o);
    ProfileOptions po;
    if (profile) po = parseProfileArgs(args);
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, mode, args);
        logger.logAndStderr("Loading clusters...");
        MergeInput in;
        hmk_profile_params params{};
        try {
            if (profile) loadProfileTables(po, params);
            in = loadMergeInput(o.inputFileName, std::string());
            if (in.clusters.empty()) throw FileFormatException("Error. The cluster file holds no clusters.");
        } catch (const FileFormatException &e) {
            logger.logAndStderr("Error. Probably wrong input file format? Run with --help for a brief description of command line parameters. Trace: \n");
            logger.logAndStderr(std::string("cz.krejciadam.hammock.FileFormatException: ") + e.what());
            return 2;
        }
        const std::vector<ClusterPtr> &clusters = in.clusters;
        const std::vector<UniqueSequencePtr> all = sequencesOf(clusters);
        logger.logAndStderr(std::to_string(clusters.size()) + " clusters of " + std::to_string(all.size()) + " sequences loaded.");
        const SequenceListSummary summary = summariseSequences(all);
        if (o.globalScorer) requireKernelLengths(summary);   // (no shift, and nothing is thresholded)
        else settleShiftAndThreshold(o, logger, summary, summary, summary, "Align");
        logScorer(o, logger);

        std::vector<UniqueSequencePtr> upload;
        const Candidates cand = appendCandidates(clusters, false, 0, upload);
        const uint32_t n = (uint32_t)upload.size(), ncl = (uint32_t)cand.slots.size();
        std::vector<uint32_t> center(ncl), width(ncl), column(n);
        std::vector<int64_t> centerSum(ncl);
        std::vector<int32_t> centerScore(n), shift(n);
        hmk_align_stats stats{};
        hmk_profile_stats pstats{};
        std::vector<uint32_t> nConserved, nMatch, counts;
        std::vector<uint8_t> passes, colFlags;
        std::vector<double> kldMatchMean, kldAllMean, ic, kldMatch, kldAll;
        std::vector<uint64_t> colStart;
        if (profile) {
            if (!po.haveMinConserved) {                                                               // Hammock.java:524-527, :1448-1452
                po.minConservedPositions = (int)javaRound(summary.meanLength() / 3);
                logger.logAndStderr("Minimal number of match states not set. Setting automatically to: " + std::to_string(po.minConservedPositions));
            }
            params.min_ic = po.minIc;
            params.max_gap_proportion = po.maxGapProportion;
            params.min_conserved_positions = po.minConservedPositions;
            params.allow_inner_gaps = po.maxInnerGaps > 0 ? 1 : 0;                                    // :1337-1341
            params.beta = 200;                                                                        // Statistics.java:21-23
            params.sigma = 10;
            params.scale = 2.88539;
        }
        logger.logAndStderr(profile ? "Aligning and profiling..." : "Aligning...");
        const auto time0 = std::chrono::steady_clock::now();
        std::unordered_map<const UniqueSequence *, std::string> rows;
        rows.reserve(n);
        if (o.globalScorer) {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(upload, true);
            alignGlobal(nc, o, upload, cand, center, centerSum, width, rows, stats);
        } else {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(upload, true);
            const int st = hmk_cluster_align_shifted(nc->get(), 0, n, cand.memberCluster.data(), ncl, o.maxShift, o.shiftPenalty, center.data(),
                                                     centerSum.data(), width.data(), nullptr, centerScore.data(), shift.data(), column.data(), &stats);
            if (st) nc->raise(st, nullptr);
            if (profile) {   // the same context, the sequences already there: the alignment's columns are the placement
                uint64_t columns = 0;
                for (uint32_t c = 0; c < ncl; c++) columns += width[c];
                nConserved.resize(ncl); nMatch.resize(ncl); passes.resize(ncl); kldMatchMean.resize(ncl); kldAllMean.resize(ncl);
                colStart.resize((size_t)ncl + 1); kldMatch.resize(n); kldAll.resize(n);
                counts.resize(columns * HMK_PROFILE_SYMBOLS); ic.resize(columns); colFlags.resize(columns);
                std::vector<uint32_t> profileWidth(ncl);
                const int ps = hmk_cluster_profile(nc->get(), 0, n, cand.memberCluster.data(), ncl, column.data(), &params, profileWidth.data(),
                                                   nConserved.data(), nMatch.data(), passes.data(), kldMatchMean.data(), kldAllMean.data(),
                                                   colStart.data(), columns, counts.data(), ic.data(), colFlags.data(), kldMatch.data(),
                                                   kldAll.data(), &pstats);
                if (ps) nc->raise(ps, nullptr);
                if (profileWidth != width) throw HammockException("the profile's widths differ from the alignment's");
            }
        }
        logger.logAndStderr("Ready. Align time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Clusters of more than one sequence: " + std::to_string(stats.n_multi) + ", pairs scored: " + std::to_string(stats.pairs_scored) +
                            ", widest alignment: " + std::to_string(stats.max_width) + ", GPU kernels: " + std::to_string(stats.kernel_ms) + " ms");
        if (profile) {
            logger.logAndStderr("Profile columns: " + std::to_string(pstats.columns) + ", GPU kernels: " + std::to_string(pstats.kernel_ms) + " ms");
            logger.logAndStderr("\nCalculating KLD...");                                             // Hammock.java:681-697
            if (pstats.omitted > 0)
                logger.logAndStderr(std::to_string(pstats.omitted) + " clusters omitted from KLD calculation because each of them only contains a single unique sequence.");
            logger.logAndStderr("Final system KLD over match state MSA positions: " + g17(pstats.system_kld_match));
            logger.logAndStderr("Final system KLD over all MSA positions: " + g17(pstats.system_kld_all));
        }
        logger.logAndStderr("Saving results to output files...");
        auto rowOf = [&](uint32_t k) {
            const std::string &s = upload[k]->getSequenceString();
            const uint32_t w = width[cand.memberCluster[k]];
            return std::string(column[k], '-') + s + std::string(w - column[k] - (uint32_t)s.size(), '-');
        };
        if (!o.globalScorer)
            for (uint32_t k = 0; k < n; k++) rows.emplace(upload[k].get(), rowOf(k));
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv", msaDir = o.workingDirectory + "/alignments_initial",
                          centersCsv = o.workingDirectory + "/cluster_centers.tsv";
        FileIOManager::writeClusterSequencesToCsv(in.lineOrder, FileIOManager::SequenceClusterIndex(clusters), seqCsv, in.labels, &rows);
        if (mkdir(msaDir.c_str(), 0777) != 0) throw HammockException("cannot create " + msaDir);
        {
            std::ofstream out(centersCsv);
            if (!out) throw HammockException("cannot write " + centersCsv);
            out << "cluster_id\tsize\tcenter\tcenter_sum\twidth\n";
            uint32_t k = 0;   // (every cluster is a candidate: slot c is cluster c, its members follow each other in upload)
            for (uint32_t c = 0; c < ncl; c++) {
                const Cluster &cl = *clusters[c];
                const uint32_t s = (uint32_t)cl.getUniqueSize();
                if (s > 1) {
                    const std::string file = msaDir + "/" + std::to_string(cl.getId()) + ".aln";
                    std::ofstream aln(file);
                    if (!aln) throw HammockException("cannot write " + file);
                    for (uint32_t t = 0; t < s; t++) aln << '>' << cl.getId() << '_' << t + 1 << '\n' << rows.at(upload[k + t].get()) << '\n';
                }
                if (s > 1 || !o.skipSingletons)
                    out << cl.getId() << '\t' << s << '\t' << upload[center[c]]->getSequenceString() << '\t' << centerSum[c] << '\t' << width[c] << '\n';
                k += s;
            }
        }
        logger.logAndStderr("Aligned cluster file in: " + seqCsv);
        logger.logAndStderr("Alignments in: " + msaDir);
        logger.logAndStderr("Centres in: " + centersCsv);
        if (profile) {
            const std::string clustersTsv = o.workingDirectory + "/cluster_profiles.tsv", positionsTsv = o.workingDirectory + "/position_profiles.tsv",
                              membersTsv = o.workingDirectory + "/member_kld.tsv";
            std::ofstream cf(clustersTsv), pf(positionsTsv), mf(membersTsv);
            if (!cf || !pf || !mf) throw HammockException("cannot write the profile files in " + o.workingDirectory);
            cf << "cluster_id\tsize\twidth\tconserved\tmatch_states\tpasses\tkld_match_mean\tkld_all_mean\n";
            pf << "cluster_id\tcolumn\tgaps\tic\tflags";
            for (int a = 0; a < 20; a++) pf << '\t' << AMINO_ACIDS[a];
            pf << '\n';
            mf << "cluster_id\tsequence\tkld_match\tkld_all\n";
            uint32_t k = 0;
            for (uint32_t c = 0; c < ncl; c++) {
                const Cluster &cl = *clusters[c];
                const uint32_t s = (uint32_t)cl.getUniqueSize();
                if (s > 1 || !o.skipSingletons) {
                    std::string states;
                    for (uint64_t g = colStart[c]; g < colStart[c + 1]; g++) states.push_back(colFlags[g] & 2 ? 'M' : '.');
                    cf << cl.getId() << '\t' << s << '\t' << width[c] << '\t' << nConserved[c] << '\t' << states << '\t' << (int)passes[c] << '\t'
                       << g17(kldMatchMean[c]) << '\t' << g17(kldAllMean[c]) << '\n';
                    for (uint64_t g = colStart[c]; g < colStart[c + 1]; g++) {
                        const uint32_t *cnt = counts.data() + g * HMK_PROFILE_SYMBOLS;
                        pf << cl.getId() << '\t' << g - colStart[c] + 1 << '\t' << cnt[20] << '\t' << g17(ic[g]) << '\t' << (int)colFlags[g];
                        for (int a = 0; a < 20; a++) pf << '\t' << cnt[a];
                        pf << '\n';
                    }
                    for (uint32_t t = 0; t < s; t++)
                        mf << cl.getId() << '\t' << upload[k + t]->getSequenceString() << '\t' << g17(kldMatch[k + t]) << '\t' << g17(kldAll[k + t]) << '\n';
                }
                k += s;
            }
            logger.logAndStderr("Cluster profiles in: " + clustersTsv);
            logger.logAndStderr("Position profiles in: " + positionsTsv);
            logger.logAndStderr("Member KLDs in: " + membersTsv);
        }
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip separation -i clusters.tsv -d dir [-x -p -m -l] [--skip_singletons]`: how well separated the clusters of a cluster file
// are, and which sequences sit closer to another cluster than to their own (hmk_cluster_separation_shifted): per sequence the mean
// ShiftedScorer score against the rest of its cluster and against the nearest other cluster -- the largest mean, the first cluster of
// the file among equal means.  Every unique sequence counts once.  Defaults of -x / -p are check's (-g is settled as there and logged,
// but nothing is thresholded).  With --skip_singletons clusters of one unique sequence are neither members nor candidates.  Writes
//   member_separation.tsv    per sequence, clusters in file order, members in cluster order: its cluster, own_sum and own_mean
//                            (= own_sum / (members - 1)), the nearest cluster with near_sum and near_mean (= near_sum / its members),
//                            margin = own_mean - near_mean, misplaced (1: own_mean < near_mean, compared exactly)
//   cluster_separation.tsv   per cluster: members, own_mean over its members (= the sum of their own_sum / (members (members - 1))),
//                            misplaced members
// A mean is one double division of two integers, printed %.4f; NA where it is undefined (the own mean of a cluster of one, the nearest
// columns of a file of one cluster).  Exit codes as check: a cluster file the loader rejects is 2.
int runSeparation(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    requireOneDevice(o, "separation", "a separation");
    requireInput(o);
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "separation", args);
        logger.logAndStderr("Loading clusters...");
        std::vector<ClusterPtr> clusters;
        try {
            clusters = FileIOManager::loadClustersFromCsv(o.inputFileName);
            if (clusters.empty()) throw FileFormatException("Error. The cluster file holds no clusters.");
        } catch (const FileFormatException &e) {
            logger.logAndStderr("Error. Probably wrong input file format? Run with --help for a brief description of command line parameters. Trace: \n");
            logger.logAndStderr(std::string("cz.krejciadam.hammock.FileFormatException: ") + e.what());
            return 2;
        }
        const std::vector<UniqueSequencePtr> all = sequencesOf(clusters);
        logger.logAndStderr(std::to_string(clusters.size()) + " clusters of " + std::to_string(all.size()) + " sequences loaded.");
        const SequenceListSummary summary = summariseSequences(all);
        settleShiftAndThreshold(o, logger, summary, summary, summary, "Separation");

        std::vector<UniqueSequencePtr> upload;
        const Candidates cand = appendCandidates(clusters, o.skipSingletons, 0, upload);
        const uint32_t n = (uint32_t)upload.size(), ncl = (uint32_t)cand.slots.size();
        std::vector<int64_t> ownSum(n), nearSum(n), clusterOwnSum(ncl);
        std::vector<uint32_t> nearCluster(n), clusterMisplaced(ncl);
        std::vector<uint8_t> misplaced(n);
        hmk_separation_stats stats{};
        logger.logAndStderr("Separation...");
        const auto time0 = std::chrono::steady_clock::now();
        if (n) {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(upload, true);
            const int st = hmk_cluster_separation_shifted(nc->get(), 0, n, cand.memberCluster.data(), ncl, o.maxShift, o.shiftPenalty, ownSum.data(),
                                                          nearSum.data(), nearCluster.data(), misplaced.data(), clusterMisplaced.data(),
                                                          clusterOwnSum.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        logger.logAndStderr("Ready. Separation time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Clusters: " + std::to_string(ncl) + ", sequences: " + std::to_string(n) + ", pairs scored: " + std::to_string(stats.pairs_scored) +
                            ", GPU kernels: " + std::to_string(stats.kernel_ms) + " ms");
        logger.logAndStderr("Saving results to output files...");
        auto fixed = [](double v) {
            char text[64];
            std::snprintf(text, sizeof text, "%.4f", v);
            return std::string(text);
        };
        const std::string membersCsv = o.workingDirectory + "/member_separation.tsv", clustersCsv = o.workingDirectory + "/cluster_separation.tsv";
        {
            std::ofstream out(membersCsv);
            if (!out) throw HammockException("cannot write " + membersCsv);
            out << "sequence\tcluster_id\tcluster_members\town_sum\town_mean\tnearest_cluster_id\tnearest_members\tnear_sum\tnear_mean\tmargin\tmisplaced\n";
            for (uint32_t k = 0; k < n; k++) {
                const Cluster &cl = *clusters[cand.slots[cand.memberCluster[k]]];
                const int64_t s = (int64_t)cl.getUniqueSize();
                const bool hasOwn = s > 1, hasNear = nearCluster[k] != UINT32_MAX;
                const double ownMean = hasOwn ? (double)ownSum[k] / (double)(s - 1) : 0.0;
                out << upload[k]->getSequenceString() << '\t' << cl.getId() << '\t' << s << '\t' << ownSum[k] << '\t' << (hasOwn ? fixed(ownMean) : "NA");
                if (!hasNear) { out << "\tNA\tNA\tNA\tNA\tNA\t" << (int)misplaced[k] << '\n'; continue; }
                const Cluster &near = *clusters[cand.slots[nearCluster[k]]];
                const double nearMean = (double)nearSum[k] / (double)(int64_t)near.getUniqueSize();
                out << '\t' << near.getId() << '\t' << near.getUniqueSize() << '\t' << nearSum[k] << '\t' << fixed(nearMean) << '\t'
                    << (hasOwn ? fixed(ownMean - nearMean) : "NA") << '\t' << (int)misplaced[k] << '\n';
            }
        }
        {
            std::ofstream out(clustersCsv);
            if (!out) throw HammockException("cannot write " + clustersCsv);
            out << "cluster_id\tmembers\town_mean\tmisplaced_members\n";
            for (uint32_t c = 0; c < ncl; c++) {
                const Cluster &cl = *clusters[cand.slots[c]];
                const int64_t s = (int64_t)cl.getUniqueSize();
                out << cl.getId() << '\t' << s << '\t' << (s > 1 ? fixed((double)clusterOwnSum[c] / (double)(s * (s - 1))) : "NA") << '\t'
                    << clusterMisplaced[c] << '\n';
            }
        }
        logger.logAndStderr("Sequences in: " + membersCsv);
        logger.logAndStderr("Clusters in: " + clustersCsv);
        logger.logAndStderr(std::to_string(stats.n_misplaced) + " of " + std::to_string(n) + " sequences are closer to another cluster than to their own");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip components -i X.fa -d dir [-g T] [--scan_to T2] [-x -p -m -f -l]`: the connected components of the neighbour graph
// {score >= t} for every t = T ... T2 from one scoring pass (hmk_components_shifted).  No cluster any other mode can form at t crosses
// a component at t (ClinkageClusterScorer.java:36-48), so this is where to read off at which threshold a data set falls apart, and
// which sequences can never cluster with anything.  Sequences in load order, as clinkage takes them; -x / -g / -p default as in
// clinkage.  Writes the stage-1 files with the components at T as clusters -- id = 1 + the smallest load-order index, multi-member
// components first in ascending id, then the singletons in ascending id, members in load order -- so that check, split, merge and
// assign take the file, and component_levels.tsv: one line per threshold.
int runComponents(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    requireOneDevice(o, "components", "a components scan");
    requireInput(o);
    requireFastaOrTab(o, "components");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "components", args);
        std::vector<std::string> labels;
        if (o.haveLabels) labels = FileIOManager::splitChar(o.labelString, ',', true);
        logger.logAndStderr("Loading input sequences...");
        std::vector<UniqueSequencePtr> sequences = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(sequences.size()) + " unique sequences loaded.");
        if (o.haveLabels) sequences = filterSequencesForLabels(sequences, labels);
        else labels = FileIOManager::getSortedLabels(sequences);
        if (sequences.empty()) throw FileFormatException("Error. No sequences (with specified labels) to cluster.");
        const SequenceListSummary summary = summariseSequences(sequences);
        settleShiftAndThreshold(o, logger, summary, summary, summary, "Components");
        const int thr = o.sequenceClusteringThreshold, thrHi = o.haveScanTo ? o.scanTo : thr;
        if (thrHi < thr || (long long)thrHi - thr > 255)
            throw CLIException("Error. --scan_to may be the threshold (-g) " + std::to_string(thr) + " up to " + std::to_string((long long)thr + 255) + ".");
        logger.logAndStderr("Parameters: max shift " + std::to_string(o.maxShift) + ", gap penalty " + std::to_string(o.shiftPenalty) + ", thresholds " +
                            std::to_string(thr) + " to " + std::to_string(thrHi));

        const uint32_t n = (uint32_t)sequences.size();
        std::vector<uint32_t> component(n);
        std::vector<hmk_component_level> levels((size_t)(thrHi - thr) + 1);
        hmk_components_stats stats{};
        logger.logAndStderr("Components...");
        const auto time0 = std::chrono::steady_clock::now();
        {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(sequences, true);
            const int st = hmk_components_shifted(nc->get(), o.maxShift, o.shiftPenalty, thr, thrHi, component.data(), levels.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        logger.logAndStderr("Ready. Components time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Pairs scored: " + std::to_string(stats.pairs_scored) + ", pairs at or above the threshold: " + std::to_string(stats.n_edges) +
                            ", GPU scoring: " + std::to_string(stats.kernel_ms) + " ms, GPU components: " + std::to_string(stats.components_ms) + " ms");
        logger.logAndStderr("Components at threshold " + std::to_string(thr) + ": " + std::to_string(stats.n_components) + ", of one sequence: " +
                            std::to_string(stats.n_singletons) + ", largest: " + std::to_string(stats.largest));
        // component[i] = the smallest index of i's component: its members follow it, in load order
        std::vector<std::vector<UniqueSequencePtr>> members(n);
        for (uint32_t i = 0; i < n; i++) members[component[i]].push_back(sequences[i]);
        std::vector<ClusterPtr> result;
        for (int multi = 1; multi >= 0; multi--)
            for (uint32_t i = 0; i < n; i++)
                if (!members[i].empty() && (members[i].size() > 1) == (multi == 1)) result.push_back(std::make_shared<Cluster>(members[i], (int)i + 1));
        logger.logAndStderr("Resulting clusers: " + std::to_string(result.size()));
        logger.logAndStderr("Saving results to output files...");
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string orderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string clustersCsv = o.workingDirectory + "/initial_clusters.tsv";
        FileIOManager::saveInitialClusters(result, seqCsv, orderedCsv, clustersCsv, labels, sequences);
        const std::string levelsCsv = o.workingDirectory + "/component_levels.tsv";
        {
            std::ofstream out(levelsCsv);
            if (!out) throw HammockException("cannot write " + levelsCsv);
            out << "threshold\tedges\tcomponents\tsingletons\tlargest\n";
            for (size_t l = 0; l < levels.size(); l++)
                out << thr + (int)l << '\t' << levels[l].n_edges << '\t' << levels[l].n_components << '\t' << levels[l].n_singletons << '\t'
                    << levels[l].largest << '\n';
        }
        logger.logAndStderr("Components as clusters in: " + clustersCsv);
        logger.logAndStderr("and: " + seqCsv);
        logger.logAndStderr("and: " + orderedCsv);
        logger.logAndStderr("Components by threshold in: " + levelsCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip density -i X.fa -d dir [-g T] [--min_neighbors K] [--scan_to T2] [--pick P] [-x -p -m -f -l]`: density clustering
// (DBSCAN on the neighbour graph {score >= t}, hmk_density_shifted) for every t = T ... T2 from one scoring pass: a sequence with at
// least K neighbours is core, clusters are the components of the core sequences, a non-core neighbour of a core sequence is border
// and joins its best core neighbour's cluster, the rest is noise.  Where `components` chains the motif families together over a few
// weak bridges, this does not.  Sequences in load order and -x / -g / -p defaults as in components.  Writes density_levels.tsv (one
// line per threshold), density_members.tsv (every sequence's kind, degree, cluster and anchor at --pick, default -g) and the stage-1
// files with the clusters at --pick -- id = 1 + the smallest core load-order index, a noise sequence a cluster of its own with id =
// 1 + its index; clusters of several sequences first in ascending id, then the single ones, members in load order -- so that they
// load back through --clusters.
int runDensity(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    bool havePick = false;
    int pick = 0, minNeighbors = 3;
    for (size_t i = 1; i + 1 < args.size(); i++) {
        if (args[i] == "--pick") { pick = javaIntegerDecode(args[++i]); havePick = true; }
        else if (args[i] == "--min_neighbors") minNeighbors = javaIntegerDecode(args[++i]);
    }
    if (minNeighbors < 0) throw CLIException("Error. --min_neighbors may not be negative.");
    requireOneDevice(o, "density", "a density clustering");
    requireInput(o);
    requireFastaOrTab(o, "density");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "density", args);
        std::vector<std::string> labels;
        if (o.haveLabels) labels = FileIOManager::splitChar(o.labelString, ',', true);
        logger.logAndStderr("Loading input sequences...");
        std::vector<UniqueSequencePtr> sequences = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(sequences.size()) + " unique sequences loaded.");
        if (o.haveLabels) sequences = filterSequencesForLabels(sequences, labels);
        else labels = FileIOManager::getSortedLabels(sequences);
        if (sequences.empty()) throw FileFormatException("Error. No sequences (with specified labels) to cluster.");
        const SequenceListSummary summary = summariseSequences(sequences);
        settleShiftAndThreshold(o, logger, summary, summary, summary, "Density clustering");
        const int thr = o.sequenceClusteringThreshold, thrHi = o.haveScanTo ? o.scanTo : thr;
        if (thrHi < thr || (long long)thrHi - thr > 255)
            throw CLIException("Error. --scan_to may be the threshold (-g) " + std::to_string(thr) + " up to " + std::to_string((long long)thr + 255) + ".");
        if (!havePick) pick = thr;
        if (pick < thr || pick > thrHi)
            throw CLIException("Error. --pick may be a threshold of the scan, " + std::to_string(thr) + " up to " + std::to_string(thrHi) + ".");
        logger.logAndStderr("Parameters: max shift " + std::to_string(o.maxShift) + ", gap penalty " + std::to_string(o.shiftPenalty) + ", thresholds " +
                            std::to_string(thr) + " to " + std::to_string(thrHi) + ", min neighbors " + std::to_string(minNeighbors) +
                            ", members and stage-1 files at " + std::to_string(pick));

        const size_t n = sequences.size(), nl = (size_t)(thrHi - thr) + 1, row = (size_t)(pick - thr) * n;
        std::vector<uint32_t> cluster(nl * n), anchor(nl * n), degree(nl * n);
        std::vector<hmk_density_level> levels(nl);
        hmk_density_stats stats{};
        logger.logAndStderr("Density clustering at " + std::to_string(nl) + " thresholds...");
        const auto time0 = std::chrono::steady_clock::now();
        {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(sequences, true);
            const int st = hmk_density_shifted(nc->get(), o.maxShift, o.shiftPenalty, thr, thrHi, minNeighbors, cluster.data(), anchor.data(), degree.data(),
                                               levels.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        logger.logAndStderr("Ready. Density clustering time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Pairs scored: " + std::to_string(stats.pairs_scored) + ", pairs at or above the threshold: " + std::to_string(stats.n_edges) +
                            ", GPU scoring: " + std::to_string(stats.kernel_ms) + " ms, GPU density clustering: " + std::to_string(stats.density_ms) + " ms");
        const hmk_density_level &at = levels[(size_t)(pick - thr)];
        logger.logAndStderr("At threshold " + std::to_string(pick) + ": core " + std::to_string(at.n_core) + ", border " + std::to_string(at.n_border) +
                            ", noise " + std::to_string(at.n_noise) + ", clusters " + std::to_string(at.n_clusters) + ", largest: " + std::to_string(at.largest));
        logger.logAndStderr("Saving results to output files...");
        const std::string levelsCsv = o.workingDirectory + "/density_levels.tsv";
        {
            std::ofstream out(levelsCsv);
            if (!out) throw HammockException("cannot write " + levelsCsv);
            out << "threshold\tedges\tcore\tborder\tnoise\tclusters\tlargest\n";
            for (size_t l = 0; l < nl; l++)
                out << thr + (int)l << '\t' << levels[l].n_edges << '\t' << levels[l].n_core << '\t' << levels[l].n_border << '\t' << levels[l].n_noise << '\t'
                    << levels[l].n_clusters << '\t' << levels[l].largest << '\n';
        }
        // the level --pick: cluster ids as in the stage-1 files, the anchor as a sequence
        const std::string membersCsv = o.workingDirectory + "/density_members.tsv";
        {
            std::ofstream out(membersCsv);
            if (!out) throw HammockException("cannot write " + membersCsv);
            out << "sequence\tkind\tdegree\tcluster\tanchor\n";
            for (size_t i = 0; i < n; i++) {
                const uint32_t c = cluster[row + i], a = anchor[row + i];
                out << sequences[i]->getSequenceString() << '\t' << (c == HMK_DENSITY_NOISE ? "noise" : a == i ? "core" : "border") << '\t' << degree[row + i]
                    << '\t' << (c == HMK_DENSITY_NOISE ? std::string("NA") : std::to_string(c + 1)) << '\t'
                    << (a == HMK_DENSITY_NOISE ? std::string("NA") : sequences[a]->getSequenceString()) << '\n';
            }
        }
        std::vector<std::vector<UniqueSequencePtr>> members(n);
        for (size_t i = 0; i < n; i++) members[cluster[row + i] == HMK_DENSITY_NOISE ? i : cluster[row + i]].push_back(sequences[i]);
        std::vector<ClusterPtr> result;
        for (int multi = 1; multi >= 0; multi--)
            for (size_t i = 0; i < n; i++)
                if (!members[i].empty() && (members[i].size() > 1) == (multi == 1)) result.push_back(std::make_shared<Cluster>(members[i], (int)i + 1));
        logger.logAndStderr("Resulting clusers at threshold " + std::to_string(pick) + ": " + std::to_string(result.size()));
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string orderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string clustersCsv = o.workingDirectory + "/initial_clusters.tsv";
        FileIOManager::saveInitialClusters(result, seqCsv, orderedCsv, clustersCsv, labels, sequences);
        logger.logAndStderr("Density clustering by threshold in: " + levelsCsv);
        logger.logAndStderr("Sequences, their kind, cluster and anchor in: " + membersCsv);
        logger.logAndStderr("Clusters (noise as single sequences) in: " + clustersCsv);
        logger.logAndStderr("and: " + seqCsv);
        logger.logAndStderr("and: " + orderedCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip sweep -i X.fa -d dir -g T --scan_to T2 [--pick P] [greedy's options]`: the greedy clustering at every threshold
// t = T ... T2 from one scoring pass (hmk_greedy_sweep; LimitedGreedySequenceClusterer.java:22,39-69 once per threshold).  Input
// loading, ordering and the defaults of -x, -g and --initial_clusters_limit are greedy's own.  Writes greedy_levels.tsv, one line per
// threshold (how many clusters, how many singletons, the largest cluster, where the reference would throw), and the stage-1 files
// of the clustering at --pick (default -g): byte for byte what `hammock-hip greedy -g P` writes.  If the reference would throw at
// P, the levels file is written, the stage-1 files are not, and the message and exit status are greedy's.
int runSweep(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    bool havePick = false;
    int pick = 0;
    for (size_t i = 1; i + 1 < args.size(); i++)
        if (args[i] == "--pick") { pick = javaIntegerDecode(args[++i]); havePick = true; }
    requireOneDevice(o, "sweep", "a sweep");
    requireInput(o);
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        std::vector<std::string> labels;
        if (o.haveLabels) labels = FileIOManager::splitChar(o.labelString, ',', true);
        if (!(o.inputType == "fasta" || o.inputType == "seq" || o.inputType == "tab"))
            throw CLIException("Error. Parameter -f value may be either \"fasta\", \"seq\" or \"tab\". No other values are allowed");
        logRunStart(logger, "sweep", args);
        // ---- greedy's loading, ordering and defaults (runSequenceClustering) -----------------------------------------------
        logger.logAndStderr("Loading input sequences...");
        if (o.inputType == "seq") throw HammockException("Error, this should have been checked.");
        std::vector<UniqueSequencePtr> sequences = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(sequences.size()) + " unique sequences loaded.");
        SequenceListSummary summary = summariseSequences(sequences);
        if (o.haveLabels) {
            sequences = filterSequencesForLabels(sequences, labels);
            summary = summariseSequences(sequences);
        }
        if (sequences.empty()) throw FileFormatException("Error. No sequences (with specified labels) to cluster.");
        if (!o.haveLabels) labels = FileIOManager::getSortedLabels(sequences);
        const std::vector<UniqueSequencePtr> initialSequences(sequences);
        settleMaxShift(o, logger, summary, summary, "");
        logger.logAndStderr("Generating input statistics...");
        FileIOManager::saveInputStatistics(sequences, labels, o.workingDirectory + "/input_statistics.tsv");
        settleThreshold(o, logger, summary, "Greedy clustering", "");
        if (!o.haveLimit) {
            o.initialClustersLimit = (int)javaRound((double)sequences.size() * 0.025);
            logger.logAndStderr("Initial greedy clusters limit not set. Setting automatically to: " + std::to_string(o.initialClustersLimit));
        }
        const int thr = o.sequenceClusteringThreshold, thrHi = o.haveScanTo ? o.scanTo : thr;
        if (thrHi < thr || (long long)thrHi - thr > 255)
            throw CLIException("Error. --scan_to may be the threshold (-g) " + std::to_string(thr) + " up to " + std::to_string((long long)thr + 255) + ".");
        if (!havePick) pick = thr;
        if (pick < thr || pick > thrHi)
            throw CLIException("Error. --pick may be a threshold of the sweep, " + std::to_string(thr) + " up to " + std::to_string(thrHi) + ".");
        logger.logAndStderr("Parameters: max shift " + std::to_string(o.maxShift) + ", gap penalty " + std::to_string(o.shiftPenalty) + ", thresholds " +
                            std::to_string(thr) + " to " + std::to_string(thrHi) + ", clusters limit " + std::to_string(o.initialClustersLimit) +
                            ", stage-1 files at " + std::to_string(pick));
        sortSequences(sequences, o.order, o.seed, labels);

        const size_t n = sequences.size(), nl = (size_t)(thrHi - thr) + 1, row = (size_t)(pick - thr) * n;
        std::vector<int32_t> cid(nl * n), order(nl * n), rank(nl * n);
        std::vector<hmk_greedy_level> levels(nl);
        hmk_greedy_sweep_stats stats{};
        logger.logAndStderr("Greedy clustering at " + std::to_string(nl) + " thresholds...");
        const auto time0 = std::chrono::steady_clock::now();
        {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(sequences, true);
            const int st = hmk_greedy_sweep(nc->get(), o.maxShift, o.shiftPenalty, thr, thrHi, o.initialClustersLimit, cid.data(), order.data(),
                                            rank.data(), levels.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        logger.logAndStderr("Ready. Sweep time: " + std::to_string(millisSince(time0)));
        double tails = 0;
        for (const hmk_greedy_level &lv : levels) tails += lv.tail_ms;
        logger.logAndStderr("Pairs scored: " + std::to_string(stats.pairs_scored) + ", pairs at or above the threshold: " + std::to_string(stats.n_edges) +
                            ", GPU scoring: " + std::to_string(stats.kernel_ms) + " ms, edges by level: " + std::to_string(stats.deal_ms) +
                            " ms, clustering tails: " + std::to_string(tails) + " ms");
        const std::string levelsCsv = o.workingDirectory + "/greedy_levels.tsv";
        {
            std::ofstream out(levelsCsv);
            if (!out) throw HammockException("cannot write " + levelsCsv);
            out << "threshold\tedges\tstatus\tclusters\tmulti_member\tsingletons\tlargest\tphase1_stop_index\n";
            for (size_t l = 0; l < nl; l++) {
                const hmk_greedy_level &lv = levels[l];
                out << thr + (int)l << '\t' << lv.n_edges << '\t' << (lv.status == HMK_OK ? std::string("ok") : "reference_would_crash:" + std::to_string(lv.crash_case))
                    << '\t' << lv.n_result_clusters << '\t' << lv.n_multi << '\t' << lv.n_singletons << '\t' << lv.largest << '\t' << lv.phase1_stop_index << '\n';
            }
        }
        logger.logAndStderr("Clusterings by threshold in: " + levelsCsv);
        const hmk_greedy_level &at = levels[(size_t)(pick - thr)];
        if (at.status != HMK_OK)   // greedy's own message (hmk_greedy_cluster's error text) and, through reportRunError, its exit status
            throw NullPointerException("the reference throws NullPointerException here (LimitedGreedySequenceClusterer.java:97/104/108): case " +
                                       std::to_string(at.crash_case) + " at index " + std::to_string(at.crash_index), at.crash_case, at.crash_index);
        // the clusters at --pick, as HipGreedySequenceClusterer::cluster builds them from one call's arrays
        std::vector<uint32_t> first(n + 1, 0);
        for (size_t k = 0; k < n; k++) first[(size_t)cid[row + k] + 1]++;
        for (size_t c = 0; c < n; c++) first[c + 1] += first[c];
        std::vector<uint32_t> slot(n);
        for (size_t k = 0; k < n; k++) slot[first[(size_t)cid[row + k]] + (size_t)rank[row + k]] = (uint32_t)k;
        std::vector<ClusterPtr> clusters((size_t)at.n_result_clusters);
        for (size_t q = 0; q < clusters.size(); q++) {
            const size_t c = (size_t)order[row + q];
            std::vector<UniqueSequencePtr> seqs;
            for (uint32_t e = first[c]; e < first[c + 1]; e++) seqs.push_back(sequences[slot[e]]);
            clusters[q] = std::make_shared<Cluster>(std::move(seqs), order[row + q]);
        }
        logger.logAndStderr("Resulting clusers at threshold " + std::to_string(pick) + ": " + std::to_string(clusters.size()));
        logger.logAndStderr("Saving results to output files...");
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string orderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string clustersCsv = o.workingDirectory + "/initial_clusters.tsv";
        FileIOManager::saveInitialClusters(clusters, seqCsv, orderedCsv, clustersCsv, labels, initialSequences);
        logger.logAndStderr("Greedy clustering results in: " + clustersCsv);
        logger.logAndStderr("and: " + seqCsv);
        logger.logAndStderr("and: " + orderedCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, true);
    }
}

// `hammock-hip orders -i X.fa -d dir [-R order] [--random_orders N] [-S seed] [--min_support S] [--pairs] [greedy's options]`: the
// greedy clustering under 1 + N orders of the input from one scoring pass (hmk_greedy_orders;
// LimitedGreedySequenceClusterer.java:22,39-69 once per order), and which of its clusters belong to the data rather than to the
// order.  The set is uploaded in the -R order (default size): order 0 is the identity, byte for byte what `hammock-hip greedy`
// clusters; orders 1..N (default 9) are -R random with the seeds S, S + 1, ...: each exactly the list `hammock-hip greedy -R random
// -S seed` clusters.  Loading and the defaults of -x, -g and --initial_clusters_limit are greedy's own.  Writes order_levels.tsv (one
// line per order), sequence_support.tsv (one line per sequence: its cluster in order 0, how many sequences share a cluster with it
// in every valid order and in at least one, its consensus cluster), with --pairs pair_support.tsv (every pair that shares a cluster
// in at least one order), and the stage-1 files with the consensus clusters -- the components of the pairs together in at least
// --min_support valid orders (default: all of them); id = 1 + the smallest place in the upload order, clusters of several sequences
// first in ascending id, then the single ones, members in upload order -- so that check, separation and align take them.
int runOrders(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    int randomOrders = 9, minSupport = 0;
    bool pairs = false;
    for (size_t i = 1; i < args.size(); i++) {
        const bool more = args.size() > i + 1;
        if (args[i] == "--random_orders" && more) randomOrders = javaIntegerDecode(args[++i]);
        else if (args[i] == "--min_support" && more) minSupport = javaIntegerDecode(args[++i]);
        else if (args[i] == "--pairs") pairs = true;
    }
    requireOneDevice(o, "orders", "an orders run");
    requireInput(o);
    if (randomOrders < 0 || randomOrders > 255) throw CLIException("Error. --random_orders may be 0 to 255.");
    if (minSupport < 0 || minSupport > randomOrders + 1)
        throw CLIException("Error. --min_support may be 0 (every valid order) up to the number of orders, " + std::to_string(randomOrders + 1) + ".");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        std::vector<std::string> labels;
        if (o.haveLabels) labels = FileIOManager::splitChar(o.labelString, ',', true);
        if (!(o.inputType == "fasta" || o.inputType == "seq" || o.inputType == "tab"))
            throw CLIException("Error. Parameter -f value may be either \"fasta\", \"seq\" or \"tab\". No other values are allowed");
        logRunStart(logger, "orders", args);
        // ---- greedy's loading and defaults (runSequenceClustering) -----------------------------------------------------------
        logger.logAndStderr("Loading input sequences...");
        if (o.inputType == "seq") throw HammockException("Error, this should have been checked.");
        std::vector<UniqueSequencePtr> sequences = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(sequences.size()) + " unique sequences loaded.");
        SequenceListSummary summary = summariseSequences(sequences);
        if (o.haveLabels) {
            sequences = filterSequencesForLabels(sequences, labels);
            summary = summariseSequences(sequences);
        }
        if (sequences.empty()) throw FileFormatException("Error. No sequences (with specified labels) to cluster.");
        if (!o.haveLabels) labels = FileIOManager::getSortedLabels(sequences);
        const std::vector<UniqueSequencePtr> initialSequences(sequences);
        settleMaxShift(o, logger, summary, summary, "");
        logger.logAndStderr("Generating input statistics...");
        FileIOManager::saveInputStatistics(sequences, labels, o.workingDirectory + "/input_statistics.tsv");
        settleThreshold(o, logger, summary, "Greedy clustering", "");
        if (!o.haveLimit) {
            o.initialClustersLimit = (int)javaRound((double)sequences.size() * 0.025);
            logger.logAndStderr("Initial greedy clusters limit not set. Setting automatically to: " + std::to_string(o.initialClustersLimit));
        }
        const int thr = o.sequenceClusteringThreshold;
        const size_t n = sequences.size(), nOrders = (size_t)randomOrders + 1;
        logger.logAndStderr("Parameters: max shift " + std::to_string(o.maxShift) + ", gap penalty " + std::to_string(o.shiftPenalty) + ", threshold " +
                            std::to_string(thr) + ", clusters limit " + std::to_string(o.initialClustersLimit) + ", orders: " + o.order + " and " +
                            std::to_string(randomOrders) + " random from seed " + std::to_string(o.seed) + ", min support " +
                            (minSupport ? std::to_string(minSupport) : std::string("every valid order")));
        sortSequences(sequences, o.order, o.seed, labels);
        // the orders: row 0 the upload order itself, row k the list -R random -S (seed + k - 1) hands to the clusterer
        std::vector<uint32_t> orders(nOrders * n);
        std::vector<std::string> orderNames(nOrders);
        {
            std::unordered_map<const UniqueSequence *, uint32_t> place;
            for (size_t i = 0; i < n; i++) {
                place[sequences[i].get()] = (uint32_t)i;
                orders[i] = (uint32_t)i;
            }
            orderNames[0] = o.order + (o.order == "random" ? ":" + std::to_string(o.seed) : "");
            for (size_t k = 1; k < nOrders; k++) {
                std::vector<UniqueSequencePtr> shuffled(initialSequences);
                const int seed = (int)((long long)o.seed + (long long)k - 1);
                sortSequences(shuffled, "random", seed, labels);
                for (size_t i = 0; i < n; i++) orders[k * n + i] = place[shuffled[i].get()];
                orderNames[k] = "random:" + std::to_string(seed);
            }
        }

        std::vector<int32_t> cid(nOrders * n);
        std::vector<hmk_greedy_order> perOrder(nOrders);
        std::vector<uint32_t> always(n), ever(n), consensus(n);
        std::vector<uint64_t> support;
        uint64_t nSupport = 0;
        hmk_greedy_orders_stats stats{};
        logger.logAndStderr("Greedy clustering under " + std::to_string(nOrders) + " orders...");
        const auto time0 = std::chrono::steady_clock::now();
        {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(sequences, true);
            for (int attempt = 0; attempt < 2; attempt++) {   // (with --pairs: once more when the first room was too small)
                if (pairs) support.resize(std::max<uint64_t>(nSupport, 16 * (uint64_t)n));
                const int st = hmk_greedy_orders(nc->get(), o.maxShift, o.shiftPenalty, thr, o.initialClustersLimit, orders.data(), (uint32_t)nOrders,
                                                 (uint32_t)minSupport, cid.data(), nullptr, nullptr, perOrder.data(), always.data(), ever.data(),
                                                 consensus.data(), pairs ? support.data() : nullptr, pairs ? support.size() : 0, &nSupport, &stats);
                if (st == HMK_ERR_CAPACITY && attempt == 0) continue;
                if (st) nc->raise(st, nullptr);
                break;
            }
        }
        logger.logAndStderr("Ready. Orders time: " + std::to_string(millisSince(time0)));
        double tails = 0;
        for (const hmk_greedy_order &po : perOrder) tails += po.tail_ms;
        logger.logAndStderr("Pairs scored: " + std::to_string(stats.pairs_scored) + ", pairs at or above the threshold: " + std::to_string(stats.n_edges) +
                            ", GPU scoring: " + std::to_string(stats.kernel_ms) + " ms, relabel: " + std::to_string(stats.relabel_ms) +
                            " ms, relabel and clustering tails: " + std::to_string(tails) + " ms, support and consensus: " +
                            std::to_string(stats.support_ms) + " ms");
        logger.logAndStderr("Valid orders: " + std::to_string(stats.n_valid) + " of " + std::to_string(stats.n_orders) + ", pairs together in at least one: " +
                            std::to_string(stats.pairs_ever) + ", in every one: " + std::to_string(stats.pairs_always));
        logger.logAndStderr("Consensus clusters: " + std::to_string(stats.n_consensus) + ", of one sequence: " + std::to_string(stats.n_consensus_singletons) +
                            ", largest: " + std::to_string(stats.consensus_largest));
        logger.logAndStderr("Saving results to output files...");
        const std::string levelsCsv = o.workingDirectory + "/order_levels.tsv";
        {
            std::ofstream out(levelsCsv);
            if (!out) throw HammockException("cannot write " + levelsCsv);
            out << "order\tstatus\tclusters\tmulti_member\tsingletons\tlargest\tpairs_together\tpairs_together_with_order_0\n";
            for (size_t k = 0; k < nOrders; k++) {
                const hmk_greedy_order &po = perOrder[k];
                out << orderNames[k] << '\t' << (po.status == HMK_OK ? std::string("ok") : "reference_would_crash:" + std::to_string(po.crash_case)) << '\t'
                    << po.n_result_clusters << '\t' << po.n_multi << '\t' << po.n_singletons << '\t' << po.largest << '\t' << po.pairs_together << '\t';
                // (pairs_with_first counts against the first VALID order: it is order 0's column only while order 0 is valid)
                if (perOrder[0].status == HMK_OK) out << po.pairs_with_first << '\n';
                else out << "NA\n";
            }
        }
        const std::string perSequence = o.workingDirectory + "/sequence_support.tsv";
        {
            std::ofstream out(perSequence);
            if (!out) throw HammockException("cannot write " + perSequence);
            out << "sequence\tcluster_in_order_0\tpartners_always\tpartners_ever\tconsensus_cluster\n";
            for (size_t i = 0; i < n; i++)
                out << sequences[i]->getSequenceString() << '\t' << (cid[i] < 0 ? std::string("NA") : std::to_string(cid[i] + 1)) << '\t' << always[i] << '\t'
                    << ever[i] << '\t' << consensus[i] + 1 << '\n';
        }
        const std::string byOrder = o.workingDirectory + "/order_clusters.tsv";
        {
            std::ofstream out(byOrder);
            if (!out) throw HammockException("cannot write " + byOrder);
            out << "sequence";
            for (size_t k = 0; k < nOrders; k++) out << '\t' << orderNames[k];
            out << '\n';
            for (size_t i = 0; i < n; i++) {   // a cluster is named by its seed: 1 + the seed's place in the upload order
                out << sequences[i]->getSequenceString();
                for (size_t k = 0; k < nOrders; k++) out << '\t' << (cid[k * n + i] < 0 ? std::string("NA") : std::to_string(cid[k * n + i] + 1));
                out << '\n';
            }
        }
        const std::string pairCsv = o.workingDirectory + "/pair_support.tsv";
        if (pairs) {
            std::sort(support.begin(), support.begin() + (long)nSupport);   // (the call's order is unspecified: by first, then second sequence)
            std::ofstream out(pairCsv);
            if (!out) throw HammockException("cannot write " + pairCsv);
            out << "sequence_1\tsequence_2\tsupport\tvalid_orders\n";
            for (uint64_t e = 0; e < nSupport; e++)
                out << sequences[HMK_EDGE_X(support[e])]->getSequenceString() << '\t' << sequences[HMK_EDGE_M(support[e])]->getSequenceString() << '\t'
                    << HMK_EDGE_SCORE(support[e]) << '\t' << stats.n_valid << '\n';
        }
        std::vector<std::vector<UniqueSequencePtr>> members(n);
        for (size_t i = 0; i < n; i++) members[consensus[i]].push_back(sequences[i]);
        std::vector<ClusterPtr> result;
        for (int multi = 1; multi >= 0; multi--)
            for (size_t i = 0; i < n; i++)
                if (!members[i].empty() && (members[i].size() > 1) == (multi == 1)) result.push_back(std::make_shared<Cluster>(members[i], (int)i + 1));
        logger.logAndStderr("Resulting clusers: " + std::to_string(result.size()));
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string orderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string clustersCsv = o.workingDirectory + "/initial_clusters.tsv";
        FileIOManager::saveInitialClusters(result, seqCsv, orderedCsv, clustersCsv, labels, initialSequences);
        logger.logAndStderr("Clusterings by order in: " + levelsCsv);
        logger.logAndStderr("Sequences and their support in: " + perSequence);
        logger.logAndStderr("Sequences and their cluster in every order in: " + byOrder);
        if (pairs) logger.logAndStderr("Pairs and their support in: " + pairCsv);
        logger.logAndStderr("Consensus clusters in: " + clustersCsv);
        logger.logAndStderr("and: " + seqCsv);
        logger.logAndStderr("and: " + orderedCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip representatives -i X.fa -d dir [-g T] [--scan_to T2] [greedy's ordering and scoring options]`: the non-redundant
// subset of the input at every threshold t = T ... T2 from one scoring pass (hmk_representatives_shifted): in greedy's order a
// sequence is a representative unless an earlier representative scores >= t with it -- the greedy incremental selection of CD-HIT
// and UCLUST.  With the default order the most abundant sequence of a family becomes its representative.  Loading, ordering and the
// defaults of -x and -g are greedy's own.  Writes representative_levels.tsv (one line per threshold), representatives.tsv (one line
// per sequence at T), representatives.fa (the representatives at T, one record per label, the label's count summed over the
// sequences nearest to that representative: it loads back through -i with the input's total count) and the stage-1 files with the
// `nearest` groups at T as clusters -- id = 1 + the representative's place in the order, groups of several sequences first in
// ascending id, then the single ones, members in the order -- so that check, separation and align take them.
int runRepresentatives(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    requireOneDevice(o, "representatives", "a selection of representatives");
    requireInput(o);
    requireFastaOrTab(o, "representatives");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "representatives", args);
        std::vector<std::string> labels;
        if (o.haveLabels) labels = FileIOManager::splitChar(o.labelString, ',', true);
        // ---- greedy's loading, ordering and defaults (runSequenceClustering) -----------------------------------------------
        logger.logAndStderr("Loading input sequences...");
        std::vector<UniqueSequencePtr> sequences = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(sequences.size()) + " unique sequences loaded.");
        SequenceListSummary summary = summariseSequences(sequences);
        if (o.haveLabels) {
            sequences = filterSequencesForLabels(sequences, labels);
            summary = summariseSequences(sequences);
        }
        if (sequences.empty()) throw FileFormatException("Error. No sequences (with specified labels) to cluster.");
        if (!o.haveLabels) labels = FileIOManager::getSortedLabels(sequences);
        const std::vector<UniqueSequencePtr> initialSequences(sequences);
        settleMaxShift(o, logger, summary, summary, "");
        settleThreshold(o, logger, summary, "Representatives", "");
        const int thr = o.sequenceClusteringThreshold, thrHi = o.haveScanTo ? o.scanTo : thr;
        if (thrHi < thr || (long long)thrHi - thr > 255)
            throw CLIException("Error. --scan_to may be the threshold (-g) " + std::to_string(thr) + " up to " + std::to_string((long long)thr + 255) + ".");
        logger.logAndStderr("Parameters: max shift " + std::to_string(o.maxShift) + ", gap penalty " + std::to_string(o.shiftPenalty) + ", thresholds " +
                            std::to_string(thr) + " to " + std::to_string(thrHi));
        sortSequences(sequences, o.order, o.seed, labels);

        const size_t n = sequences.size(), nl = (size_t)(thrHi - thr) + 1;
        std::vector<uint32_t> covered(nl * n), nearest(nl * n);
        std::vector<int32_t> score(nl * n);
        std::vector<hmk_representative_level> levels(nl);
        hmk_representatives_stats stats{};
        logger.logAndStderr("Representatives at " + std::to_string(nl) + " thresholds...");
        const auto time0 = std::chrono::steady_clock::now();
        {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(sequences, true);
            const int st = hmk_representatives_shifted(nc->get(), o.maxShift, o.shiftPenalty, thr, thrHi, covered.data(), nearest.data(), score.data(),
                                                       levels.data(), &stats);
            if (st) nc->raise(st, nullptr);
        }
        logger.logAndStderr("Ready. Representatives time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Pairs scored: " + std::to_string(stats.pairs_scored) + ", pairs at or above the threshold: " + std::to_string(stats.n_edges) +
                            ", GPU scoring: " + std::to_string(stats.kernel_ms) + " ms, GPU selection: " + std::to_string(stats.select_ms) + " ms, rounds: " +
                            std::to_string(stats.rounds_total));
        logger.logAndStderr("Representatives at threshold " + std::to_string(thr) + ": " + std::to_string(stats.n_representatives) + ", without a neighbour: " +
                            std::to_string(stats.n_isolated) + ", largest group: " + std::to_string(stats.largest));
        logger.logAndStderr("Saving results to output files...");
        const std::string levelsCsv = o.workingDirectory + "/representative_levels.tsv";
        {
            std::ofstream out(levelsCsv);
            if (!out) throw HammockException("cannot write " + levelsCsv);
            out << "threshold\tedges\trepresentatives\tisolated\tlargest\n";
            for (size_t l = 0; l < nl; l++)
                out << thr + (int)l << '\t' << levels[l].n_edges << '\t' << levels[l].n_representatives << '\t' << levels[l].n_isolated << '\t'
                    << levels[l].largest << '\n';
        }
        // the level -g: row 0 of the arrays
        const std::string perSequence = o.workingDirectory + "/representatives.tsv";
        {
            std::ofstream out(perSequence);
            if (!out) throw HammockException("cannot write " + perSequence);
            out << "sequence\trepresentative\tcovered_by\tnearest\tscore\n";
            for (size_t i = 0; i < n; i++) {
                const bool rep = nearest[i] == i;
                out << sequences[i]->getSequenceString() << '\t' << (rep ? 1 : 0) << '\t' << sequences[covered[i]]->getSequenceString() << '\t'
                    << sequences[nearest[i]]->getSequenceString() << '\t' << (rep ? std::string("NA") : std::to_string(score[i])) << '\n';
            }
        }
        std::vector<std::vector<UniqueSequencePtr>> members(n);
        for (size_t i = 0; i < n; i++) members[nearest[i]].push_back(sequences[i]);
        const std::string fasta = o.workingDirectory + "/representatives.fa";
        {
            std::ofstream out(fasta);
            if (!out) throw HammockException("cannot write " + fasta);
            for (size_t i = 0; i < n; i++) {
                if (members[i].empty()) continue;
                for (const std::string &label : labels) {
                    long long count = 0;
                    for (const UniqueSequencePtr &s : members[i])
                        for (const auto &e : s->getLabelsMap())
                            if (e.first == label) count += e.second;
                    if (count > 0) out << '>' << i + 1 << '|' << count << '|' << label << '\n' << sequences[i]->getSequenceString() << '\n';
                }
            }
        }
        std::vector<ClusterPtr> result;
        for (int multi = 1; multi >= 0; multi--)
            for (size_t i = 0; i < n; i++)
                if (!members[i].empty() && (members[i].size() > 1) == (multi == 1)) result.push_back(std::make_shared<Cluster>(members[i], (int)i + 1));
        logger.logAndStderr("Resulting clusers: " + std::to_string(result.size()));
        const std::string seqCsv = o.workingDirectory + "/initial_clusters_sequences.tsv";
        const std::string orderedCsv = o.workingDirectory + "/initial_clusters_sequences_original_order.tsv";
        const std::string clustersCsv = o.workingDirectory + "/initial_clusters.tsv";
        FileIOManager::saveInitialClusters(result, seqCsv, orderedCsv, clustersCsv, labels, initialSequences);
        logger.logAndStderr("Representatives by threshold in: " + levelsCsv);
        logger.logAndStderr("Sequences and their representatives in: " + perSequence);
        logger.logAndStderr("Representatives in: " + fasta);
        logger.logAndStderr("Groups as clusters in: " + clustersCsv);
        logger.logAndStderr("and: " + seqCsv);
        logger.logAndStderr("and: " + orderedCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip survey -i X.fa -d dir [-g T] [--database known.fa] [-x -p -m -f -l]`: what the pair scores of a set look like, before a
// threshold is chosen for any other mode (hmk_score_survey_shifted): the histogram of the scores, every sequence's best partner and its
// number of partners at -g.  Without --database the triangle over the input in load order (every unordered pair, as components scores
// them); with it the input's sequences are the queries and the database's the references (search's rectangle).  -x / -g / -p default as
// in components (search's lists with --database).  The histogram window is settled here: first the HMK_SURVEY_MAX_BINS scores ending at
// the longest length x the matrix's largest cell; if a pair fell outside, once more at [score_min, score_max] of the first call.
int runSurvey(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    requireOneDevice(o, "survey", "a survey");
    requireInput(o);
    requireFastaOrTab(o, "survey");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "survey", args);
        std::vector<std::string> labels;
        if (o.haveLabels) labels = FileIOManager::splitChar(o.labelString, ',', true);
        logger.logAndStderr("Loading input sequences...");
        std::vector<UniqueSequencePtr> sequences = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(sequences.size()) + " unique sequences loaded.");
        if (o.haveLabels) sequences = filterSequencesForLabels(sequences, labels);
        if (sequences.empty()) throw FileFormatException("Error. No sequences (with specified labels) to survey.");
        std::vector<UniqueSequencePtr> all(sequences);
        if (o.haveDatabase) {
            logger.logAndStderr("Loading reference sequences...");
            const std::vector<UniqueSequencePtr> references = loadSequences(o, o.database);
            logger.logAndStderr(std::to_string(references.size()) + " unique reference sequences loaded.");
            if (references.empty()) throw FileFormatException("Error. No reference sequences to survey against.");
            all.insert(all.end(), references.begin(), references.end());
        }
        const SequenceListSummary summary = summariseSequences(all);
        settleShiftAndThreshold(o, logger, summary, summary, summariseSequences(sequences), "Survey");
        const int thr = o.sequenceClusteringThreshold;
        logger.logAndStderr("Parameters: max shift " + std::to_string(o.maxShift) + ", gap penalty " + std::to_string(o.shiftPenalty) + ", threshold " +
                            std::to_string(thr));
        int maxCell = INT32_MIN;
        for (auto &row : FileIOManager::loadScoringMatrix(o.matrixFile)) for (int v : row) maxCell = std::max(maxCell, v);

        const uint32_t nq = (uint32_t)sequences.size(), n = (uint32_t)all.size();
        const uint32_t r0 = o.haveDatabase ? nq : 0, r1 = o.haveDatabase ? n : nq;
        std::vector<uint64_t> hist(HMK_SURVEY_MAX_BINS);
        std::vector<int32_t> bestScore(nq);
        std::vector<uint32_t> bestIndex(nq), degree(nq);
        hmk_survey_stats stats{};
        int lo = summary.maxLength * maxCell - (HMK_SURVEY_MAX_BINS - 1);
        double kernelMs = 0;
        logger.logAndStderr("Survey...");
        const auto time0 = std::chrono::steady_clock::now();
        {
            const std::shared_ptr<NativeContext> nc = contextReady.get();
            nc->setSequences(all, false);
            int st = hmk_score_survey_shifted(nc->get(), 0, nq, r0, r1, o.maxShift, o.shiftPenalty, thr, lo, HMK_SURVEY_MAX_BINS, hist.data(),
                                              bestScore.data(), bestIndex.data(), degree.data(), &stats);
            if (st) nc->raise(st, nullptr);
            kernelMs = stats.kernel_ms;
            if (stats.n_below || stats.n_above) {   // a pair outside the window: the scores' own range, if it fits one
                const long long span = (long long)stats.score_max - stats.score_min + 1;
                if (span > HMK_SURVEY_MAX_BINS)
                    throw CLIException("Error. The pair scores span " + std::to_string(span) + " values (" + std::to_string(stats.score_min) + " to " +
                                       std::to_string(stats.score_max) + "): more than the " + std::to_string(HMK_SURVEY_MAX_BINS) +
                                       " a survey's histogram holds (HMK_SURVEY_MAX_BINS).");
                lo = stats.score_min;
                logger.logAndStderr("Scores outside the first window. Scoring again for the scores " + std::to_string(stats.score_min) + " to " +
                                    std::to_string(stats.score_max));
                hmk_survey_stats again{};
                st = hmk_score_survey_shifted(nc->get(), 0, nq, r0, r1, o.maxShift, o.shiftPenalty, thr, lo, (uint32_t)span, hist.data(), nullptr,
                                              nullptr, nullptr, &again);
                if (st) nc->raise(st, nullptr);
                if (again.n_below || again.n_above || again.score_min != stats.score_min || again.score_max != stats.score_max)
                    throw HammockException("the second survey call does not repeat the first one's score range");
                kernelMs += again.kernel_ms;
            }
        }
        logger.logAndStderr("Ready. Survey time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Pairs scored: " + std::to_string(stats.pairs_scored) + ", pairs at or above the threshold: " +
                            std::to_string(stats.n_at_or_above) + ", GPU kernels: " + std::to_string(kernelMs) + " ms");
        logger.logAndStderr("Saving results to output files...");
        const std::string histCsv = o.workingDirectory + "/score_histogram.tsv", nnCsv = o.workingDirectory + "/nearest_neighbors.tsv";
        {
            std::ofstream out(histCsv);
            if (!out) throw HammockException("cannot write " + histCsv);
            out << "score\tpairs\tpairs_at_or_above\tsequences_best\tsequences_best_at_or_above\n";
            if (stats.pairs_scored) {
                const size_t span = (size_t)((long long)stats.score_max - stats.score_min + 1);
                std::vector<uint64_t> pairs(span), best(span), pairsUp(span), bestUp(span);
                for (size_t k = 0; k < span; k++) pairs[k] = hist[(size_t)((long long)stats.score_min + (long long)k - lo)];
                for (uint32_t q = 0; q < nq; q++)
                    if (bestIndex[q] != 0xFFFFFFFFu) best[(size_t)((long long)bestScore[q] - stats.score_min)]++;
                uint64_t a = 0, b = 0;
                for (size_t k = span; k-- > 0;) { a += pairs[k]; b += best[k]; pairsUp[k] = a; bestUp[k] = b; }
                for (size_t k = 0; k < span; k++)
                    out << (long long)stats.score_min + (long long)k << '\t' << pairs[k] << '\t' << pairsUp[k] << '\t' << best[k] << '\t' << bestUp[k] << '\n';
            }
        }
        {
            std::ofstream out(nnCsv);
            if (!out) throw HammockException("cannot write " + nnCsv);
            out << "sequence\tbest_partner\tbest_score\tneighbors_at_threshold\n";
            for (uint32_t q = 0; q < nq; q++) {
                out << sequences[q]->getSequenceString() << '\t';
                if (bestIndex[q] == 0xFFFFFFFFu) out << "NA\tNA";
                else out << all[bestIndex[q]]->getSequenceString() << '\t' << bestScore[q];
                out << '\t' << degree[q] << '\n';
            }
        }
        logger.logAndStderr("Score histogram in: " + histCsv);
        logger.logAndStderr("Nearest neighbours in: " + nnCsv);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

// `hammock-hip io-selftest ...`: exposes the loaders / orderings to the CPU test-suite (no GPU involved)
// `hammock-hip scan -i peptides.fa --targets proteins.fa -d dir ...`: where on the targets do the peptides sit?  Every peptide of -i
// slides along every target as scoreWithShift(seq1 = peptide, seq2 = target) slides it (ShiftedScorer.java:67-85; hmk_scan_shifted):
// one line per (peptide, target) whose best window reaches -g -- or, with --all_windows, per window that does -- to
// <dir>/scan_hits.tsv, the coverage of the targets' residues by those lines to target_coverage.tsv (targets with a hit only), one line
// per target to target_summary.tsv.  Rows are sorted by (target, offset, peptide in load order): two runs write the same bytes.
// Defaults: -x and -g as greedy derives them from the peptides (Hammock.java:394-397, 1421-1434), -p 0.
int runScan(const std::vector<std::string> &args) {
    Options o;
    parseCommonArgs(args, o);
    parseModeArgs(args, o, -1);
    std::string targetsFile;
    bool allWindows = false;
    for (size_t i = 1; i < args.size(); i++) {
        if (args[i] == "--targets" && args.size() > i + 1) targetsFile = args[++i];
        else if (args[i] == "--all_windows") allWindows = true;
    }
    requireOneDevice(o, "scan", "a scan");
    requireInput(o);
    if (targetsFile.empty()) throw CLIException("Error. Parameter targets file (--targets) missing with no default.");
    requireFastaOrTab(o, "scan");
    makeOutputDirectory(o, o.parentDir);
    Logger logger(o.workingDirectory + "/run.log", false);
    try {
        ContextFuture contextReady = beginRun(o, logger, false);
        logRunStart(logger, "scan", args);
        logger.logAndStderr("Loading peptides...");
        const std::vector<UniqueSequencePtr> peptides = loadSequences(o, o.inputFileName);
        logger.logAndStderr(std::to_string(peptides.size()) + " unique peptides loaded.");
        if (peptides.empty()) throw FileFormatException("Error. No peptides to scan with.");
        requireOccurrences(peptides, "Error in file " + o.inputFileName);
        logger.logAndStderr("Loading targets...");
        TargetSet targets;
        try {
            targets = loadTargetsFromFasta(targetsFile, HMK_MAX_LEN + 1, HMK_TARGET_MAX_LEN);
        } catch (const TargetFormatError &e) {
            throw FileFormatException(e.what());
        }
        logger.logAndStderr(std::to_string(targets.size()) + " targets loaded, " + std::to_string(targets.residues.size()) + " residues.");
        if (targets.size() == 0) throw FileFormatException("Error. No targets to scan.");
        const SequenceListSummary summary = summariseSequences(peptides);
        settleShiftAndThreshold(o, logger, summary, summary, summary, "Scan");

        const std::shared_ptr<NativeContext> nc = contextReady.get();
        hmk_ctx *c = nc->get();
        nc->setSequences(peptides, true);
        const uint32_t nq = (uint32_t)peptides.size(), nt = (uint32_t)targets.size();
        int st = hmk_set_targets(c, targets.residues.data(), targets.offsets.data(), nt);
        if (st) nc->raise(st, nullptr);
        logger.logAndStderr("Scanning...");
        const auto time0 = std::chrono::steady_clock::now();
        std::vector<hmk_scan_hit> hits(1 << 16);
        std::vector<uint32_t> covCount(targets.residues.size());
        std::vector<uint64_t> covSize(targets.residues.size());
        hmk_scan_stats stats{};
        const uint32_t flags = allWindows ? HMK_SCAN_ALL_WINDOWS : 0u;
        st = hmk_scan_shifted(c, 0, nq, 0, nt, o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold, flags, hits.data(), hits.size(),
                              covCount.data(), covSize.data(), &stats);
        if (st == HMK_ERR_CAPACITY) {
            hits.resize(stats.n_hits);
            st = hmk_scan_shifted(c, 0, nq, 0, nt, o.maxShift, o.shiftPenalty, o.sequenceClusteringThreshold, flags, hits.data(), hits.size(),
                                  covCount.data(), covSize.data(), &stats);
        }
        if (st) nc->raise(st, nullptr);
        hits.resize(stats.n_hits);
        std::sort(hits.begin(), hits.end(), [](const hmk_scan_hit &a, const hmk_scan_hit &b) {
            return a.target != b.target ? a.target < b.target : a.offset != b.offset ? a.offset < b.offset : a.query < b.query;
        });
        logger.logAndStderr("Ready. Scan time: " + std::to_string(millisSince(time0)));
        logger.logAndStderr("Windows scored: " + std::to_string(stats.windows_scored) + " (" + std::to_string(stats.windows_packed) + " on byte lanes), windows at or above the threshold: " +
                            std::to_string(stats.window_hits) + ", hits reported: " + std::to_string(stats.n_hits) + ", GPU kernels: " +
                            std::to_string(stats.kernel_ms) + " ms");
        const std::string hitsFile = o.workingDirectory + "/scan_hits.tsv", coverageFile = o.workingDirectory + "/target_coverage.tsv",
                          summaryFile = o.workingDirectory + "/target_summary.tsv";
        struct PerTarget { uint64_t hits = 0; int best = INT_MIN; std::unordered_set<uint32_t> peptides; };
        std::vector<PerTarget> per(nt);
        {
            std::ofstream out(hitsFile);
            if (!out) throw HammockException("cannot write " + hitsFile);
            out << "peptide\tcount\ttarget\tstart\tscore\tsegment\n";
            for (const hmk_scan_hit &h : hits) {
                const std::string &pep = peptides[h.query]->getSequenceString();
                const int64_t n = (int64_t)targets.length(h.target);
                std::string segment;
                for (int64_t i = 0; i < (int64_t)pep.size(); i++) {
                    const int64_t pos = (int64_t)h.offset + i;
                    segment.push_back(pos >= 0 && pos < n ? AMINO_ACIDS[targets.residues[targets.offsets[h.target] + (uint64_t)pos]] : '-');
                }
                out << pep << '\t' << peptides[h.query]->size() << '\t' << targets.names[h.target] << '\t' << h.offset + 1 << '\t' << h.score << '\t'
                    << segment << '\n';
                PerTarget &pt = per[h.target];
                pt.hits++;
                pt.best = std::max(pt.best, (int)h.score);
                pt.peptides.insert(h.query);
            }
        }
        {
            std::ofstream cov(coverageFile), sum(summaryFile);
            if (!cov) throw HammockException("cannot write " + coverageFile);
            if (!sum) throw HammockException("cannot write " + summaryFile);
            cov << "target\tposition\tresidue\thits\tcount\n";
            sum << "target\tlength\thits\tpeptides\tbest_score\tcovered_positions\n";
            for (uint32_t t = 0; t < nt; t++) {
                uint64_t covered = 0;
                for (uint64_t k = targets.offsets[t]; k < targets.offsets[t + 1]; k++) {
                    covered += covCount[k] != 0;
                    if (per[t].hits)
                        cov << targets.names[t] << '\t' << k - targets.offsets[t] + 1 << '\t' << AMINO_ACIDS[targets.residues[k]] << '\t' << covCount[k] << '\t'
                            << covSize[k] << '\n';
                }
                sum << targets.names[t] << '\t' << targets.length(t) << '\t' << per[t].hits << '\t' << per[t].peptides.size() << '\t'
                    << (per[t].hits ? std::to_string(per[t].best) : std::string("NA")) << '\t' << covered << '\n';
            }
        }
        logger.logAndStderr("Scan results in: " + hitsFile + ", " + coverageFile + ", " + summaryFile);
        logger.logWithTime("Program successfully ended.");
        return 0;
    } catch (...) {
        return reportRunError(logger, false);
    }
}

int ioSelftest(const std::vector<std::string> &args) {
    if (args.size() >= 3 && args[1] == "matrix") {
        for (auto &row : FileIOManager::loadScoringMatrix(args[2])) {
            for (size_t c = 0; c < row.size(); c++) std::cout << (c ? " " : "") << row[c];
            std::cout << "\n";
        }
        return 0;
    }
    if (args.size() >= 3 && args[1] == "targets") {  // targets <fasta>: what `scan --targets` loads, one "name<TAB>length<TAB>letters" per record
        const TargetSet set = loadTargetsFromFasta(args[2], HMK_MAX_LEN + 1, HMK_TARGET_MAX_LEN);
        for (size_t t = 0; t < set.size(); t++) {
            std::cout << set.names[t] << "\t" << set.length(t) << "\t";
            for (uint64_t k = set.offsets[t]; k < set.offsets[t + 1]; k++) std::cout << AMINO_ACIDS[set.residues[k]];
            std::cout << "\n";
        }
        return 0;
    }
    if (args.size() >= 5 && args[1] == "sequences") {  // sequences <fasta|tab> <file> <order> [seed]
        auto seqs = args[2] == "tab" ? FileIOManager::loadUniqueSequencesFromTable(args[3])
                                     : FileIOManager::loadUniqueSequencesFromFasta(args[3]);
        const std::vector<std::string> labels = FileIOManager::getSortedLabels(seqs);
        sortSequences(seqs, args[4], args.size() > 5 ? javaIntegerDecode(args[5]) : 42, labels);
        std::cout << "labels";
        for (auto &l : labels) std::cout << "\t" << l;
        std::cout << "\n";
        for (auto &s : seqs) std::cout << s->getSequenceString() << "\t" << FileIOManager::sequenceLine(*s, labels) << "\n";
        return 0;
    }
    if (args.size() >= 8 && args[1] == "writers") {  // writers <fasta|tab> <file> <order> <seed> <clusters.tsv> <out dir>
        // clusters.tsv: one cluster per line, "id<TAB>SEQ,SEQ,..." in list order; the result files are written twice, by the
        // reference's three calls in a row (<out dir>/serial) and side by side (<out dir>/side)
        auto seqs = args[2] == "tab" ? FileIOManager::loadUniqueSequencesFromTable(args[3])
                                     : FileIOManager::loadUniqueSequencesFromFasta(args[3]);
        const std::vector<std::string> labels = FileIOManager::getSortedLabels(seqs);
        const std::vector<UniqueSequencePtr> initial(seqs);
        FileIOManager::saveInputStatistics(seqs, labels, args[7] + "/input_statistics.tsv");
        sortSequences(seqs, args[4], javaIntegerDecode(args[5]), labels);
        std::unordered_map<std::string, UniqueSequencePtr> byString;
        for (auto &q : seqs) byString[q->getSequenceString()] = q;
        auto build = [&]() {
            std::vector<ClusterPtr> clusters;
            for (const std::string &line : FileIOManager::readLines(args[6])) {
                const std::vector<std::string> f = FileIOManager::splitChar(line, '\t', true);
                if (f.size() < 2) continue;
                std::vector<UniqueSequencePtr> members;
                for (const std::string &m : FileIOManager::splitChar(f[1], ',', true)) members.push_back(byString.at(m));
                clusters.push_back(std::make_shared<Cluster>(members, javaIntegerDecode(f[0])));
            }
            return clusters;
        };
        std::vector<ClusterPtr> a = build(), b = build();
        FileIOManager::saveClusterSequencesToCsv(a, args[7] + "/serial/initial_clusters_sequences.tsv", labels);
        FileIOManager::saveClusterSequencesToCsvOrdered(a, args[7] + "/serial/initial_clusters_sequences_original_order.tsv", labels, initial);
        FileIOManager::SaveClustersToCsv(a, args[7] + "/serial/initial_clusters.tsv", labels);
        FileIOManager::saveInitialClusters(b, args[7] + "/side/initial_clusters_sequences.tsv", args[7] + "/side/initial_clusters_sequences_original_order.tsv",
                                           args[7] + "/side/initial_clusters.tsv", labels, initial);
        return 0;
    }
    if (args.size() >= 3 && args[1] == "clusters") {  // clusters <cluster file>: what loadClustersFromCsv makes of it
        for (auto &cl : FileIOManager::loadClustersFromCsv(args[2]))
            for (auto &s : cl->getSequences()) std::cout << cl->getId() << "\t" << s->getSequenceString() << "\t" << s->size() << "\n";
        return 0;
    }
    std::cerr << "usage: hammock-hip io-selftest matrix <file> | targets <fasta> | sequences <fasta|tab> <file> <order> [seed] | "
                 "writers <fasta|tab> <file> <order> <seed> <clusters.tsv> <out dir> | clusters <cluster file>\n";
    return 2;
}

// `hammock-hip api-selftest <known_answers.tsv> <matrix>`: drives the mirrored C++ classes
// (ShiftedScorer, LocalAlignmentScorer, Cluster, HipGreedySequenceClusterer) the way a unit test of the
// reference would -- one sequenceScore / cluster call at a time -- and prints the results.
// Lines: "shifted seq1 seq2 X p" | "local seq1 seq2 open ext" | "greedy thr maxShift penalty maxClusters seq..."
int apiSelftest(const std::vector<std::string> &args) {
    if (args.size() < 3) { std::cerr << "usage: hammock-hip api-selftest <cases.tsv> <matrix file> [device]\n"; return 2; }
    const auto M = FileIOManager::loadScoringMatrix(args[2]);
    const int device = args.size() > 3 ? javaIntegerDecode(args[3]) : 0;
    for (const std::string &line : FileIOManager::readLines(args[1])) {
        const std::vector<std::string> f = FileIOManager::splitChar(line, '\t', true);
        if (f.empty() || f[0].empty() || f[0][0] == '#') continue;
        try {
            if (f[0] == "shifted" && f.size() >= 5) {
                ShiftedScorer sc(M, javaIntegerDecode(f[4]), javaIntegerDecode(f[3]), device);
                const AligningScorerResult r = sc.scoreWithShift(std::make_shared<UniqueSequence>(f[1]),
                                                                 std::make_shared<UniqueSequence>(f[2]));
                std::cout << "shifted\t" << f[1] << "\t" << f[2] << "\t" << r.getScore() << "\t" << r.getShift() << "\n";
            } else if (f[0] == "local" && f.size() >= 5) {
                LocalAlignmentScorer sc(M, javaIntegerDecode(f[3]), javaIntegerDecode(f[4]), device);
                std::cout << "local\t" << f[1] << "\t" << f[2] << "\t"
                          << sc.sequenceScore(std::make_shared<UniqueSequence>(f[1]), std::make_shared<UniqueSequence>(f[2])) << "\n";
            } else if (f[0] == "greedy" && f.size() >= 6) {
                auto scorer = std::make_shared<ShiftedScorer>(M, javaIntegerDecode(f[3]), javaIntegerDecode(f[2]), device);
                HipGreedySequenceClusterer clusterer(scorer, javaIntegerDecode(f[1]), javaIntegerDecode(f[4]));
                std::vector<UniqueSequencePtr> seqs;
                for (size_t k = 5; k < f.size(); k++) seqs.push_back(std::make_shared<UniqueSequence>(f[k]));
                std::ostringstream os;
                os << "greedy";
                for (auto &cl : clusterer.cluster(seqs)) {
                    os << "\t" << cl->getId() << ":";
                    for (size_t k = 0; k < cl->getSequences().size(); k++)
                        os << (k ? "," : "") << cl->getSequences()[k]->getSequenceString();
                }
                std::cout << os.str() << "\n";
            }
        } catch (const DataException &e) {
            std::cout << f[0] << "\tDataException\t" << e.what() << "\n";
        } catch (const NullPointerException &e) {
            std::cout << f[0] << "\tNullPointerException\tcase " << e.crashCase << " index " << e.crashIndex << "\n";
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // 10^6 sequences are 4 x 10^6 small allocations made on 16 threads: glibc grows a thread's arena by `top_pad` (128 KB) per
    // mprotect call, and every such call stops the page faults of all other threads; larger steps, fewer calls
    mallopt(M_TOP_PAD, 64 << 20);
    std::vector<std::string> args(argv + 1, argv + argc);
    if (args.empty() || args[0] == "--help" || args[0] == "-h") { printHelp(); return args.empty() ? 2 : 0; }
    try {
        if (args[0] == "greedy") return runSequenceClustering(args, false);
        if (args[0] == "clinkage") return runSequenceClustering(args, true);
        if (args[0] == "search") return runSearch(args);
        if (args[0] == "assign") return runAssign(args);
        if (args[0] == "continue") return runContinue(args);
        if (args[0] == "match") return runMatch(args);
        if (args[0] == "merge") return runMerge(args);
        if (args[0] == "check") return runCheck(args);
        if (args[0] == "split") return runSplit(args);
        if (args[0] == "components") return runComponents(args);
        if (args[0] == "density") return runDensity(args);
        if (args[0] == "sweep") return runSweep(args);
        if (args[0] == "orders") return runOrders(args);
        if (args[0] == "representatives") return runRepresentatives(args);
        if (args[0] == "align") return runAlign(args);
        if (args[0] == "profile") return runAlign(args, true);
        if (args[0] == "survey") return runSurvey(args);
        if (args[0] == "separation") return runSeparation(args);
        if (args[0] == "scan") return runScan(args);
        if (args[0] == "io-selftest") return ioSelftest(args);
        if (args[0] == "dump-matrix") {   // the default matrix in the text format FileIOManager.loadScoringMatrix reads
            std::cout << "# BLOSUM62 substitution matrix (public NCBI table), 24 x 24, order " << AMINO_ACIDS << "\n"
                      << "# default of hammock-hip greedy (-m), same text format Hammock's -m files use\n  ";
            for (int c = 0; c < 24; c++) std::cout << "  " << AMINO_ACIDS[c];
            std::cout << "\n";
            for (int r = 0; r < 24; r++) {
                std::cout << AMINO_ACIDS[r];
                for (int c = 0; c < 24; c++) {
                    const std::string v = std::to_string(BLOSUM62[r][c]);
                    std::cout << std::string(3 - v.size(), ' ') << v;
                }
                std::cout << "\n";
            }
            return 0;
        }
        if (args[0] == "api-selftest") return apiSelftest(args);
        std::cerr << "hammock-hip implements Hammock's initial-clustering modes `greedy` and `clinkage` (modes full, cluster, "
                     "compare drive external HMM tools and are outside the scope of the MI355X hot path); got mode \"" << args[0] << "\"\n";
        return 2;
    } catch (const CLIException &e) {  // Hammock.java:146-147
        std::cerr << "Error in command line arguments: " << e.what() << std::endl;
        return 2;
    } catch (const FileFormatException &e) {
        std::cerr << "Error. Probably wrong input file format? Run with --help for a brief description of command line parameters. Trace: \n"
                  << e.what() << std::endl;
        return 3;
    } catch (const std::exception &e) {
        std::cerr << "Error. Run with --help for a brief description of command line parameters. Trace: \n" << e.what() << std::endl;
        return 6;
    }
}
